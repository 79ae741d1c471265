"""The prover's constraint check (include/zkgpu_stark.h zkgpu_stark_check_*):
the quotient program on the trace domain, before stage 3's commit, names the
rows that break the AIR.  Against the CPU oracle (tests/check_cases.py
oracle_check with the challenge the prover reports): clean and corrupted
traces under both memory plans, the streamed stage 1, an unsatisfiable program,
the compiled kernels against the interpreter.  A checked proof is the
unchecked proof bit for bit, and with the check off a proof queues what it
queued before."""
import copy
import uuid

import numpy as np
import pytest

import check_cases as cc

pytestmark = pytest.mark.gpu

P = cc.P
N = 1 << 10
CORRUPT = {"row0": (0,), "row517": (517,), "last": (N - 1,), "two": (3, N - 1)}


def _inst(blow=1, kind=False):
    import bench
    return bench.stark_instance(10, blow, 100, 16, kind)


def _oracle(inst, rows=()):
    from oracle.stark_prover import OracleStark
    o = OracleStark(inst)
    o.witness()
    cc.corrupt(o, rows)
    trace = o.S[0].copy()
    return o, trace, o.prove()


@pytest.fixture(scope="module")
def clean(oracle):
    """{blowup: (oracle prover after prove(), its trace, its proof)} (shared, not modified but for S[10])"""
    return {blow: _oracle(_inst(blow)) for blow in (1, 2)}


@pytest.fixture(scope="module")
def corrupted(oracle):
    return {name: _oracle(_inst(), rows) for name, rows in CORRUPT.items()}


def _modes():
    from zkgpu.stark import MEM_LEAN, MEM_RESIDENT
    return {"resident": MEM_RESIDENT, "lean": MEM_LEAN}


def _same_as_oracle(res, o):
    want = cc.oracle_check(o, res["alpha"])
    assert (res["n_bad"], res["rows"], res["value"]) == want
    return want


def _replayed_alpha(g, proof):
    """the check's challenge from the proof's own roots"""
    from zkgpu.stark import Transcript
    t = Transcript()
    t.put(g.verkey())
    t.put(g.publics())
    t.put(np.array([int(x) for x in proof["root1"]], np.uint64))
    t.get_field(), t.get_field()
    t.put(np.array([int(x) for x in proof["root2"]], np.uint64))
    t.get_field(), t.get_field()
    return [int(x) for x in t.get_field()]


# ---------------------------------------------------------------- 1. clean traces
@pytest.mark.parametrize("mode", ["resident", "lean"])
@pytest.mark.parametrize("blow", [1, 2])
def test_clean_trace(zkgpu, clean, monkeypatch, blow, mode):
    from zkgpu.stark import CHECK_REPORT, GpuStark
    monkeypatch.delenv("ZKGPU_LEAN_KEEP_COLS", raising=False)
    o, _, proof = clean[blow]
    g = GpuStark(o.inst, mode=_modes()[mode])
    try:
        g.check_set(CHECK_REPORT)
        g.witness()
        assert g.check_result()["ran"] == 0
        assert g.prove() == proof
        res = g.check_result()
        assert res["ran"] == 1 and res["n_bad"] == 0 and res["rows"] == [] and res["value"] == [0, 0, 0]
        assert res["alpha"] == _replayed_alpha(g, proof) and any(res["alpha"])
        assert "ZKGPU_CHECK_CONSTRAINTS" in g.timers()
        _same_as_oracle(res, o)
    finally:
        g.close()


# ---------------------------------------------------------------- 2. corrupted traces
@pytest.mark.parametrize("mode", ["resident", "lean"])
@pytest.mark.parametrize("name", sorted(CORRUPT))
def test_corrupted_trace(zkgpu, corrupted, monkeypatch, name, mode):
    from zkgpu import ZkgpuError
    from zkgpu.stark import CHECK_OFF, CHECK_REPORT, CHECK_STOP, GpuStark
    monkeypatch.delenv("ZKGPU_LEAN_KEEP_COLS", raising=False)
    o, trace, proof = corrupted[name]
    rows = sorted(CORRUPT[name])
    g = GpuStark(o.inst, mode=_modes()[mode])
    try:
        g.check_set(CHECK_REPORT)
        g.set_cm1(trace)
        assert g.prove() == proof  # the proof of that trace, as the oracle's
        res = g.check_result()
        assert res["ran"] == 1 and res["alpha"] == _replayed_alpha(g, proof)
        n_bad, bad, value = _same_as_oracle(res, o)
        assert (n_bad, bad) == (len(rows), rows) and any(value)
        # STOP: prove fails at the check with the first row in its message, and the result still reads
        g.check_set(CHECK_STOP)
        g.set_cm1(trace)
        with pytest.raises(ZkgpuError, match=r"constraint check: %d of the 2\^10 = 1024 rows of the trace break the "
                                             r"AIR; the first is row %d " % (len(rows), rows[0])):
            g.prove()
        assert g.check_result() == res
        assert "ZKGPU_CHECK_CONSTRAINTS" in g.timers() and "STARK_STEP_3_LDE" not in g.timers()
        # the trace was not consumed, under the lean plan either: the same trace proves with the check off
        g.check_set(CHECK_OFF)
        assert g.prove() == proof
        assert g.check_result()["ran"] == 0
    finally:
        g.close()


# ---------------------------------------------------------------- 3. streamed stage 1
def test_streamed_stage1(zkgpu, corrupted, monkeypatch):
    from zkgpu.stark import CHECK_REPORT, GpuStark, MEM_LEAN
    monkeypatch.setenv("ZKGPU_STREAM_COLS", "8")
    monkeypatch.delenv("ZKGPU_STREAM_FAIL_BATCH", raising=False)
    monkeypatch.delenv("ZKGPU_LEAN_KEEP_COLS", raising=False)
    o, trace, proof = corrupted["two"]
    g = GpuStark(o.inst, mode=MEM_LEAN)
    try:
        g.check_set(CHECK_REPORT)
        g.set_cm1(trace)
        assert g.prove() == proof
        want = g.check_result()
        assert g.prove_from_rows(trace) == proof
        assert g.check_result() == want and want["rows"] == [3, N - 1]
    finally:
        g.close()


# ---------------------------------------------------------------- 4. an unsatisfiable program
def test_unsatisfiable_program(zkgpu, oracle):
    """the zkEVM-shaped instance is no satisfiable AIR: every count, row and value as the oracle's"""
    from zkgpu.stark import CHECK_REPORT, GpuStark, MEM_RESIDENT
    o, _, proof = _oracle(_inst(1, "zkevm"))
    g = GpuStark(o.inst, mode=MEM_RESIDENT)
    try:
        g.check_set(CHECK_REPORT)
        g.witness()
        assert g.prove() == proof
        res = g.check_result()
        n_bad, bad, value = _same_as_oracle(res, o)
        assert n_bad > 16 and len(bad) == 16 and any(value)
    finally:
        g.close()


# ---------------------------------------------------------------- 5. the compiled path
def test_compiled_kernels_equal_the_interpreter(zkgpu, monkeypatch):
    """2^16 rows: the rewritten program runs as run-time compiled kernels (its own cache entries)"""
    from zkgpu.stark import CHECK_REPORT, GpuStark, MEM_RESIDENT
    from zkgpu.synthetic import SyntheticStark
    r = 40961
    g = GpuStark(SyntheticStark(n_bits=16), mode=MEM_RESIDENT)
    try:
        g.witness()
        trace = g.get_cm1()
        trace[r, 2] = (int(trace[r, 2]) + 1) % P
        g.set_cm1(trace)
        g.check_set(CHECK_REPORT)
        out = []
        for jit in ("1", "0"):
            monkeypatch.setenv("ZKGPU_ZXP_JIT", jit)
            proof = g.prove_raw()
            out.append((g.check_result(), proof))
        assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1])
        assert out[0][0]["ran"] == 1 and out[0][0]["n_bad"] == 1 and out[0][0]["rows"] == [r]
    finally:
        g.close()


# ---------------------------------------------------------------- 6. off means off
def test_off_means_off(zkgpu, clean):
    from zkgpu.stark import CHECK_OFF, CHECK_REPORT, GpuStark, MEM_RESIDENT
    o, _, _ = clean[1]
    never = GpuStark(o.inst, mode=MEM_RESIDENT)
    g = GpuStark(o.inst, mode=MEM_RESIDENT)
    zkgpu.prof_enable(True)
    try:
        never.witness()
        zkgpu.prof_reset()
        p0 = never.prove_raw()
        k0 = zkgpu.prof_kernels()
        g.witness()
        g.check_set(CHECK_REPORT)
        zkgpu.prof_reset()
        p1 = g.prove_raw()
        k1 = zkgpu.prof_kernels()
        assert g.check_result()["ran"] == 1
        g.check_set(CHECK_OFF)
        zkgpu.prof_reset()
        p2 = g.prove_raw()
        k2 = zkgpu.prof_kernels()
        assert g.check_result()["ran"] == 0
        assert np.array_equal(p0, p1) and np.array_equal(p0, p2)
        assert list(g.timers()) == list(never.timers()) and "ZKGPU_CHECK_CONSTRAINTS" not in g.timers()
        assert sorted(k2) == sorted(k0)
        assert {"k_nz_count", "k_nz_emit"} <= set(k1) and not {"k_nz_count", "k_nz_emit"} & set(k0)
    finally:
        zkgpu.prof_enable(False)
        never.close()
        g.close()


# ---------------------------------------------------------------- 7. refusals
def test_refusals(zkgpu):
    from zkgpu import ZkgpuError
    from zkgpu import synthetic as sy
    from zkgpu.stark import CHECK_REPORT, GpuStark, MEM_RESIDENT, ShmComm
    inst = _inst()
    g = GpuStark(inst, mode=MEM_RESIDENT)
    try:
        with pytest.raises(ZkgpuError, match="check_set: unknown mode 3"):
            g.check_set(3)
    finally:
        g.close()
    # a quotient program that reads the quotient pieces: refused with the rewrite's message, the check stays off
    bad = copy.deepcopy(inst)
    p = bad.programs["step42ns"]
    k = len(p.opnd)
    a = p.o(sy.COL, sy.SEC_CM4_2NS, 0, 0)
    assert a == k
    p.op(sy.ADD, p.o(sy.TMP1, 0, 0, 0), a, a)
    g = GpuStark(bad, mode=MEM_RESIDENT)
    try:
        with pytest.raises(ZkgpuError, match="check_set: step42ns: zxp_to_n_domain: operand %d names section 8; the "
                                             "check is off" % k):
            g.check_set(CHECK_REPORT)
        g.witness()
        g.prove_raw()
        assert g.check_result()["ran"] == 0 and "ZKGPU_CHECK_CONSTRAINTS" not in g.timers()
    finally:
        g.close()
    comm = ShmComm("/zkgpu_chk_%s" % uuid.uuid4().hex[:12], 1, 0, capacity=1 << 20)
    try:
        g = GpuStark(inst, comm=comm)
        try:
            with pytest.raises(ZkgpuError, match="check_set is single-GPU only"):
                g.check_set(CHECK_REPORT)
        finally:
            g.close()
    finally:
        comm.close()
