"""The constraint check's naming (include/zkgpu_stark.h
zkgpu_stark_check_names_set / _terms / _named): which terms of step42ns's
combination fail at the rows the check lists.  Against the CPU oracle
(tests/split_cases.py oracle_terms with the challenge the prover reports):
corrupted traces under both memory plans in REPORT and STOP, the clean trace
(every slot empty, the proof unchanged bit for bit, one more kernel), naming
off (the kernels the check queued before), 2^16 rows behind the compiled
kernels, the streamed stage 1, the refusals, the driver.

The zkEVM-shaped instance (about 4600 terms, every row failing) multiplies its
accumulator once by another challenge into a slot nothing reads: the split
drops that product (csrc/zxp_split.cpp, the spoiled slots)."""
import os
import subprocess
import uuid

import numpy as np
import pytest

import check_cases as cc
import split_cases as sc

pytestmark = pytest.mark.gpu

P = cc.P
N = 1 << 10
CORRUPT = {"row0": (0,), "row517": (517,), "last": (N - 1,), "two": (3, N - 1)}


def _inst(blow=1, kind=False):
    import bench
    return bench.stark_instance(10, blow, 100, 16, kind)


def _oracle(inst, rows=(), cols=(2,)):
    from oracle.stark_prover import OracleStark
    o = OracleStark(inst)
    o.witness()
    for r in rows:
        for c in cols:
            o.S[0][r, c] = (int(o.S[0][r, c]) + 1) % P
    trace = o.S[0].copy()
    return o, trace, o.prove()


@pytest.fixture(scope="module")
def corrupted(oracle):
    return {name: _oracle(_inst(), rows) for name, rows in CORRUPT.items()}


@pytest.fixture(scope="module")
def clean(oracle):
    return _oracle(_inst())


def _modes():
    from zkgpu.stark import MEM_LEAN, MEM_RESIDENT
    return {"resident": MEM_RESIDENT, "lean": MEM_LEAN}


def _named_as_oracle(g, o, res, max_terms=None):
    """every slot of the last check against the oracle's terms -> [(ids, values)] of the listed rows"""
    terms, v = sc.oracle_terms(o, res["alpha"])
    assert np.array_equal(g.check_terms(), terms)
    out = []
    for slot in range(16):
        ids, vals, n = g.check_named(slot, max_terms)
        if slot < len(res["rows"]):
            want_ids, want_vals = sc.named(terms, v, res["rows"][slot])
            assert n == len(want_ids) and n > 0
            k = n if max_terms is None else min(n, max_terms)
            assert (ids, vals) == (want_ids[:k], want_vals[:k])
        else:
            assert (ids, vals, n) == ([], [], 0)
        out.append((ids, vals))
    if max_terms is None and res["rows"]:
        assert sc.combine(terms, out[0][1], res["alpha"], out[0][0]) == res["value"]
    return out


# ---------------------------------------------------------------- 1. corrupted traces
@pytest.mark.parametrize("mode", ["resident", "lean"])
@pytest.mark.parametrize("name", sorted(CORRUPT))
def test_corrupted_trace(zkgpu, corrupted, monkeypatch, name, mode):
    from zkgpu import ZkgpuError
    from zkgpu.stark import CHECK_REPORT, CHECK_STOP, GpuStark
    monkeypatch.delenv("ZKGPU_LEAN_KEEP_COLS", raising=False)
    o, trace, proof = corrupted[name]
    rows = sorted(CORRUPT[name])
    g = GpuStark(o.inst, mode=_modes()[mode])
    try:
        g.check_set(CHECK_REPORT)
        g.check_names_set(True)
        g.set_cm1(trace)
        assert g.prove() == proof
        res = g.check_result()
        assert (res["n_bad"], res["rows"], res["value"]) == cc.oracle_check(o, res["alpha"]) and res["rows"] == rows
        got = _named_as_oracle(g, o, res)
        assert [ids for ids, _ in got[:len(rows)]] == [[0]] * len(rows)  # triple 0's identity, nothing else
        g.check_set(CHECK_STOP)
        g.set_cm1(trace)
        with pytest.raises(ZkgpuError, match=r"constraint check: %d of the 2\^10 = 1024 rows of the trace break the "
                                             r"AIR; the first is row %d \(zkgpu_stark_check_result lists the lowest "
                                             r"16\); failing terms there: 0 \(zkgpu_stark_check_named\)$"
                                             % (len(rows), rows[0])):
            g.prove()
        assert g.check_result() == res
        assert _named_as_oracle(g, o, res) == got
    finally:
        g.close()


def test_two_identities_at_one_row(zkgpu, oracle):
    from zkgpu import ZkgpuError
    from zkgpu.stark import CHECK_REPORT, CHECK_STOP, GpuStark, MEM_RESIDENT
    o, trace, proof = _oracle(_inst(), (600,), (2, 5))
    g = GpuStark(o.inst, mode=MEM_RESIDENT)
    try:
        g.check_set(CHECK_REPORT)
        g.check_names_set(True)
        g.set_cm1(trace)
        assert g.prove() == proof
        res = g.check_result()
        assert res["rows"] == [600]
        got = _named_as_oracle(g, o, res)
        assert got[0][0] == [0, 1]
        assert _named_as_oracle(g, o, res, max_terms=1)[0][0] == [0]  # max below the count
        g.check_set(CHECK_STOP)
        g.set_cm1(trace)
        with pytest.raises(ZkgpuError, match=r"; failing terms there: 0 1 \(zkgpu_stark_check_named\)$"):
            g.prove()
    finally:
        g.close()


# ---------------------------------------------------------------- 2. an unsatisfiable program
def test_unsatisfiable_program(zkgpu, oracle):
    """the zkEVM-shaped instance (n_bad > 16, many terms per row): all 16 rows as the oracle's,
    and with max below the count"""
    from zkgpu.stark import CHECK_REPORT, GpuStark, MEM_RESIDENT
    inst = _inst(1, "zkevm")
    g = GpuStark(inst, mode=MEM_RESIDENT)
    try:
        g.check_set(CHECK_REPORT)
        g.check_names_set(True)
        o, _, proof = _oracle(inst)
        g.witness()
        assert g.prove() == proof
        res = g.check_result()
        assert res["n_bad"] > 16 and len(res["rows"]) == 16
        got = _named_as_oracle(g, o, res)
        assert all(len(ids) > 1 for ids, _ in got)
        _named_as_oracle(g, o, res, max_terms=2)
    finally:
        g.close()


# ---------------------------------------------------------------- 3. clean trace; naming off
def test_clean_trace_and_naming_off(zkgpu, clean):
    from zkgpu.stark import CHECK_REPORT, GpuStark, MEM_RESIDENT
    o, trace, proof = clean
    plain = GpuStark(o.inst, mode=MEM_RESIDENT)   # checked, naming never set
    g = GpuStark(o.inst, mode=MEM_RESIDENT)
    zkgpu.prof_enable(True)
    try:
        plain.check_set(CHECK_REPORT)
        plain.witness()
        zkgpu.prof_reset()
        p0 = plain.prove_raw()
        k0 = zkgpu.prof_kernels()
        g.check_set(CHECK_REPORT)
        g.check_names_set(True)
        g.witness()
        zkgpu.prof_reset()
        p1 = g.prove_raw()
        k1 = zkgpu.prof_kernels()
        res = g.check_result()
        assert res["ran"] == 1 and res["n_bad"] == 0
        assert [g.check_named(s) for s in range(16)] == [([], [], 0)] * 16
        g.check_names_set(False)
        zkgpu.prof_reset()
        p2 = g.prove_raw()
        k2 = zkgpu.prof_kernels()
        assert g.check_result() == res
        assert np.array_equal(p0, p1) and np.array_equal(p0, p2) and g.parse(p1) == proof
        assert "k_zxp_eval_rows" in k1 and sorted(set(k1) - {"k_zxp_eval_rows"}) == sorted(set(k0))
        assert sorted(set(k2)) == sorted(set(k0)) and {"k_nz_count", "k_nz_emit"} <= set(k0)
        assert list(g.timers()) == list(plain.timers())
    finally:
        zkgpu.prof_enable(False)
        plain.close()
        g.close()


# ---------------------------------------------------------------- 4. behind the compiled kernels
def test_2p16_rows(zkgpu):
    from zkgpu.stark import CHECK_REPORT, GpuStark, MEM_RESIDENT
    from zkgpu.synthetic import SyntheticStark
    r = 40961
    g = GpuStark(SyntheticStark(n_bits=16), mode=MEM_RESIDENT)
    zkgpu.prof_enable(True)
    try:
        g.witness()
        trace = g.get_cm1()
        trace[r, 2] = (int(trace[r, 2]) + 1) % P
        g.set_cm1(trace)
        zkgpu.prof_reset()
        g.prove_raw()  # unchecked: what the proof's own programs launch
        jit0, eval0 = zkgpu.prof_query("k_zxp_jit")[0], zkgpu.prof_query("k_zxp_eval")[0]
        g.check_set(CHECK_REPORT)
        g.check_names_set(True)
        zkgpu.prof_reset()
        g.prove_raw()
        kernels = zkgpu.prof_kernels()
        res = g.check_result()
        assert res["n_bad"] == 1 and res["rows"] == [r]
        # the check itself ran as a compiled kernel, not on the interpreter; the names on k_zxp_eval_rows
        assert jit0 > 0 and zkgpu.prof_query("k_zxp_jit")[0] == jit0 + 1
        assert zkgpu.prof_query("k_zxp_eval")[0] == eval0 == 0
        assert "k_zxp_eval_rows" in kernels and zkgpu.prof_query("k_zxp_eval_rows")[0] == 1
        ids, vals, n = g.check_named(0)
        assert (ids, n) == ([0], 1)
        assert sc.combine(g.check_terms(), vals, res["alpha"], ids) == res["value"]
        assert g.check_named(1) == ([], [], 0)
    finally:
        zkgpu.prof_enable(False)
        g.close()


# ---------------------------------------------------------------- 5. streamed stage 1
def test_streamed_stage1(zkgpu, corrupted, monkeypatch):
    from zkgpu.stark import CHECK_REPORT, GpuStark, MEM_LEAN
    monkeypatch.setenv("ZKGPU_STREAM_COLS", "8")
    monkeypatch.delenv("ZKGPU_STREAM_FAIL_BATCH", raising=False)
    monkeypatch.delenv("ZKGPU_LEAN_KEEP_COLS", raising=False)
    o, trace, proof = corrupted["two"]
    g = GpuStark(o.inst, mode=MEM_LEAN)
    try:
        g.check_set(CHECK_REPORT)
        g.check_names_set(True)
        g.set_cm1(trace)
        assert g.prove() == proof
        want = [g.check_named(s) for s in range(16)]
        assert g.prove_from_rows(trace) == proof
        assert [g.check_named(s) for s in range(16)] == want and want[1] == ([0], want[1][1], 1)
    finally:
        g.close()


# ---------------------------------------------------------------- 6. refusals
def test_refusals(zkgpu, oracle):
    from zkgpu import ZkgpuError
    from zkgpu.stark import CHECK_REPORT, GpuStark, MEM_RESIDENT, ShmComm
    inst = _inst()
    g = GpuStark(inst, mode=MEM_RESIDENT)
    try:
        g.check_set(CHECK_REPORT)
        g.witness()
        g.prove_raw()
        with pytest.raises(ZkgpuError, match="check_named: the last proof ran no check with naming on"):
            g.check_named(0)
        g.check_names_set(True)
        with pytest.raises(ZkgpuError, match="check_named: slot 16 of 16"):
            g.check_named(16)
    finally:
        g.close()
    # a program the split refuses (its store to q twice): naming stays off, the rows are still reported
    import copy
    bad = copy.deepcopy(inst)
    p = bad.programs["step42ns"]
    last = [int(x) for x in p.arrays()[0][-1]]
    p.op(*last)
    g = GpuStark(bad, mode=MEM_RESIDENT)
    try:
        g.check_set(CHECK_REPORT)
        with pytest.raises(ZkgpuError, match="check_names_set: step42ns: zxp_split: instruction %d is a second store "
                                             "to q; naming is off" % (len(p.arrays()[0]) - 1)):
            g.check_names_set(True)
        g.witness()
        trace = g.get_cm1()
        trace[77, 2] = (int(trace[77, 2]) + 1) % P
        g.set_cm1(trace)
        g.prove_raw()
        res = g.check_result()
        assert res["ran"] == 1 and res["n_bad"] == 1 and res["rows"] == [77]
        with pytest.raises(ZkgpuError, match="check_named: the last proof ran no check with naming on"):
            g.check_named(0)
    finally:
        g.close()
    comm = ShmComm("/zkgpu_nam_%s" % uuid.uuid4().hex[:12], 1, 0, capacity=1 << 20)
    try:
        g = GpuStark(inst, comm=comm)
        try:
            with pytest.raises(ZkgpuError, match="check_names_set is single-GPU only"):
                g.check_names_set(True)
        finally:
            g.close()
    finally:
        comm.close()


# ---------------------------------------------------------------- 7. the driver
def test_driver_names_the_term(oracle, tmp_path):
    import zkgpu.starkinfo as zs
    from oracle.stark_prover import OracleStark
    from test_starkinfo import DRIVER
    from zkgpu.synthetic import SyntheticStark
    inst = SyntheticStark(n_bits=8, t=2, m=1, n_queries=8)
    o = OracleStark(inst)
    o.witness()
    bad = o.S[0].copy()
    bad[77, 2] = (int(bad[77, 2]) + 1) % P
    cfg = zs.write_inputs(str(tmp_path), inst, o.S[4], o.S[9], o.const_nodes, bad, o.publics)
    r = subprocess.run([DRIVER, "--check-trace", cfg], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert ("constraint check: 1 of the 2^8 = 256 rows of the trace break the AIR; the first is row 77 "
            "(zkgpu_stark_check_result lists the lowest 16); failing terms there: 0 (zkgpu_stark_check_named)"
            ) in r.stderr, r.stderr
    assert not os.path.exists(tmp_path / "out" / "batch_proof.zkin.json")
