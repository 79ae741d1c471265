"""calculateZ's diagnosis (include/zkgpu_stark.h zkgpu_stark_z_diag): a grand
product that does not close names the values that keep it open.  The
SyntheticStark permutation check (n_perms = 1) with cells of (C, D) altered,
against the pure-Python reference on the trace's (A, B) / (C, D) tuples
(tests/multiset_cases.py), at blowup 1 and 2 under both memory plans; a clean
trace proves as the oracle and queues no kernel of the comparison."""
import re
import uuid

import numpy as np
import pytest

import multiset_cases as mc

pytestmark = pytest.mark.gpu

P = mc.P
N = 1 << 10
KERNELS = {"k_multiset_insert", "k_multiset_flag", "k_multiset_emit"}


@pytest.fixture(scope="module")
def clean(oracle):
    """{blowup bits: (instance, the oracle's trace, its proof)}"""
    from oracle.stark_prover import OracleStark
    from zkgpu.synthetic import SyntheticStark
    out = {}
    for blow in (1, 2):
        inst = SyntheticStark(n_bits=10, blowup_bits=blow, n_perms=1)
        o = OracleStark(inst)
        o.witness()
        out[blow] = (inst, o.S[0].copy(), o.prove())
    return out


def _modes():
    from zkgpu.stark import MEM_LEAN, MEM_RESIDENT
    return {"resident": MEM_RESIDENT, "lean": MEM_LEAN}


def _alter(inst, trace, cells):
    """cells: (row, column index into the permutation's A B C D, new value or None = + 1)"""
    bad = trace.copy()
    for row, k, v in cells:
        c = inst.perms[0]["cols"][k]
        bad[row, c] = (int(bad[row, c]) + 1) % P if v is None else v
    return bad


def _fails(g, inst, prove, want):
    """prove() fails at calculateZ with the diagnosis `want` in the message and in z_diag()"""
    from zkgpu import ZkgpuError
    with pytest.raises(ZkgpuError) as e:
        prove()
    msg = str(e.value)
    z = len(inst.z_ctx) - 1
    assert "calculateZ: grand product %d does not close (1 of %d do not): " % (z, len(inst.z_ctx)) in msg, msg
    tail = msg.split("do not): ")[1]
    for side, key in (("num", "num"), ("den", "den")):
        row, cn, cd = want[key][0]
        assert "%d value(s) of %s unmatched, the first at row %d (%d in num, %d in den)" % (
            want["n_" + key], side, row, cn, cd) in tail, msg
    d = g.z_diag()
    assert (d["ran"], d["z"], d["n_open"]) == (1, z, 1)
    assert {k: d[k] for k in want} == want
    return msg


@pytest.mark.parametrize("mode", ["resident", "lean"])
@pytest.mark.parametrize("blow", [1, 2])
def test_clean_trace(zkgpu, clean, monkeypatch, blow, mode):
    from zkgpu.stark import GpuStark
    monkeypatch.delenv("ZKGPU_LEAN_KEEP_COLS", raising=False)
    inst, trace, proof = clean[blow]
    g = GpuStark(inst, mode=_modes()[mode])
    zkgpu.prof_enable(True)
    try:
        g.witness()
        assert np.array_equal(g.get_cm1(), trace)
        g.set_cm1(trace)
        zkgpu.prof_reset()
        assert g.prove() == proof
        assert g.z_diag()["ran"] == 0
        ks = set(zkgpu.prof_kernels())
        assert ks and not KERNELS & ks
    finally:
        zkgpu.prof_enable(False)
        g.close()


@pytest.mark.parametrize("mode", ["resident", "lean"])
@pytest.mark.parametrize("blow", [1, 2])
def test_altered_cells(zkgpu, clean, monkeypatch, blow, mode):
    from zkgpu.stark import GpuStark
    monkeypatch.delenv("ZKGPU_LEAN_KEEP_COLS", raising=False)
    inst, trace, proof = clean[blow]
    rot = inst.PERM_ROT
    g = GpuStark(inst, mode=_modes()[mode])
    zkgpu.prof_enable(True)
    try:
        g.witness()
        got = g.get_cm1()
        assert np.array_equal(got, trace)
        for r in (0, 517, N - 1):
            bad = _alter(inst, got, [(r, 2, None)])  # one cell of C
            want = mc.perm_reference(inst, bad)
            # the orphan of (A, B) is the row C's row was rotated from
            assert want == {"n_num": 1, "num": [((r + rot) % N, 1, 0)], "n_den": 1, "den": [(r, 0, 1)]}
            g.set_cm1(bad)
            zkgpu.prof_reset()
            _fails(g, inst, g.prove, want)
            assert KERNELS <= set(zkgpu.prof_kernels())
        # one value 2 against 0: the (C, D) cells of two rows become one tuple no row of (A, B) holds
        bad = _alter(inst, got, [(40, 2, 12345), (40, 3, 67890), (900, 2, 12345), (900, 3, 67890)])
        want = mc.perm_reference(inst, bad)
        assert want["n_den"] == 1 and want["den"] == [(40, 0, 2)] and want["n_num"] == 2
        assert want["num"] == [(40 + rot, 1, 0), (900 + rot, 1, 0)]
        g.set_cm1(bad)
        _fails(g, inst, g.prove, want)
        # the failed proof leaves a prover that proves: the clean trace, the oracle's proof, no diagnosis
        g.set_cm1(trace)
        assert g.prove() == proof
        assert g.z_diag()["ran"] == 0
    finally:
        zkgpu.prof_enable(False)
        g.close()


@pytest.mark.parametrize("mode", ["resident", "lean"])
def test_streamed_stage1(zkgpu, clean, monkeypatch, mode):
    from zkgpu.stark import GpuStark
    monkeypatch.setenv("ZKGPU_STREAM_COLS", "8")
    monkeypatch.delenv("ZKGPU_STREAM_FAIL_BATCH", raising=False)
    monkeypatch.delenv("ZKGPU_LEAN_KEEP_COLS", raising=False)
    inst, trace, proof = clean[1]
    bad = _alter(inst, trace, [(517, 2, None)])
    want = mc.perm_reference(inst, bad)
    g = GpuStark(inst, mode=_modes()[mode])
    try:
        g.set_cm1(bad)
        first = _fails(g, inst, g.prove, want)
        again = _fails(g, inst, lambda: g.prove_from_rows(bad), want)
        assert re.sub(r"^\S+ failed: ", "", again) == re.sub(r"^\S+ failed: ", "", first)
        assert g.prove_from_rows(trace) == proof
        assert g.z_diag()["ran"] == 0
    finally:
        g.close()


def test_sharded_handle_is_refused(zkgpu, clean):
    from zkgpu import ZkgpuError
    from zkgpu.stark import GpuStark, ShmComm
    inst, _, _ = clean[1]
    comm = ShmComm("/zkgpu_zdg_%s" % uuid.uuid4().hex[:12], 1, 0, capacity=1 << 20)
    try:
        g = GpuStark(inst, comm=comm)
        try:
            with pytest.raises(ZkgpuError, match="single-GPU provers only"):
                g.z_diag()
        finally:
            g.close()
    finally:
        comm.close()
