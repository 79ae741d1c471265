"""The prover's probe (include/zkgpu_stark.h zkgpu_stark_probe_*) and the
gather it rests on (zkgpu_gather_rows_dev, csrc/stark.hip k_gather_rows).

A probed proof records sampled rows of every section each stage program reads
and writes, from the section table in force at that moment.  Under every
memory plan -- the lean plan's in-place extensions in many batches, its
two-region stage-1 tree, the streamed stage 1 -- the records must equal the
oracle's bit for bit, record by record, the proof must still equal the
oracle's, and the checker (tests/zxp_rows.py) must find nothing.  With no
probe set a proof launches nothing new and returns the same bytes."""
import copy

import numpy as np
import pytest

import zxp_rows as zr
from test_oracle_rows import sample_rows

pytestmark = pytest.mark.gpu

CASES = {"config4": (1, False), "zkevm_shaped": (1, "zkevm"), "blowup2": (2, False)}


def _inst(case):
    import bench
    blow, kind = CASES[case]
    return bench.stark_instance(10, blow, 100, 16, kind)


def _rows(inst, seed=5):
    rng = np.random.default_rng(seed)
    return (sample_rows(1 << inst.n_bits, rng, n_random=32)[0],
            sample_rows(1 << inst.n_bits_ext, rng, n_random=32)[0])


@pytest.fixture(scope="module")
def want(oracle):
    """{case: (records, proof, publics)} of the oracle (shared, never modified)"""
    from oracle.stark_prover import OracleStark
    out = {}
    for case in CASES:
        inst = _inst(case)
        o = OracleStark(inst)
        o.witness()
        recs, proof = zr.oracle_probe(o, *_rows(inst))
        out[case] = (recs, proof, o.publics.copy())
    return out


def _probed_proof_equals_oracle(g, inst, want_case, prove):
    recs, proof, publics = want_case
    g.probe_set(*_rows(inst))
    assert g.probe_size() == (0, 0)
    assert prove() == proof
    got = g.probe()
    assert len(got) == g.probe_size()[0] == len(recs)
    zr.assert_same_probe(got, recs)
    assert np.array_equal(g.publics(), publics)
    stats = {}
    assert zr.check_probe(inst, got, publics, stats) == []
    assert len(stats) == 5 and all(s["nonzero"] and s["rows"] >= 32 for s in stats.values())
    assert "ZKGPU_PROBE_READBACK" in g.timers()
    return got


# ---------------------------------------------------------------- 1. gather
@pytest.mark.parametrize("ncols", [1, 7, 751])
def test_gather_rows(zkgpu, ncols):
    import torch
    n = 1 << 12
    ld = n + 5
    g = torch.Generator(device="cuda")
    g.manual_seed(ncols)
    src = torch.randint(0, 2**63 - 1, (ncols, ld), dtype=torch.int64, device="cuda", generator=g)
    rng = np.random.default_rng(ncols)
    rows = np.concatenate([[ld - 1, n - 1, n - 1, 0], rng.integers(0, ld, 200)]).astype(np.int64)
    assert rows[0] > rows[1] and rows[1] == rows[2]  # descending, one repeat
    drows = torch.from_numpy(rows).cuda()
    out = torch.full((rows.size, ncols), -1, dtype=torch.int64, device="cuda")
    zkgpu.gather_rows_dev(out, src, ld, ncols, drows, rows.size)
    torch.cuda.synchronize()
    assert torch.equal(out, src[:, drows].t())
    before = out.clone()
    zkgpu.gather_rows_dev(out, src, ld, ncols, drows, 0)
    zkgpu.gather_rows_dev(out, src, ld, 0, drows, rows.size)
    torch.cuda.synchronize()
    assert torch.equal(out, before)
    with pytest.raises(zkgpu.ZkgpuError, match="null pointer"):
        zkgpu.gather_rows_dev(None, src, ld, ncols, drows, rows.size)


# ---------------------------------------------------------------- 2. probe == oracle
@pytest.mark.parametrize("case", ["config4", "zkevm_shaped"])
def test_probe_equals_oracle_resident(zkgpu, want, case):
    from zkgpu.stark import GpuStark, MEM_RESIDENT
    inst = _inst(case)
    g = GpuStark(inst, mode=MEM_RESIDENT)
    try:
        g.witness()
        _probed_proof_equals_oracle(g, inst, want[case], g.prove)
    finally:
        g.close()


@pytest.mark.parametrize("case", ["config4", "zkevm_shaped"])
@pytest.mark.parametrize("batch,keep", [(0, None), (7, "0"), (7, "45"), (0, "100000")],
                         ids=["batch_default-keep_auto", "batch7-keep0", "batch7-keep_part", "keep_all"])
def test_probe_equals_oracle_lean(zkgpu, want, monkeypatch, case, batch, keep):
    """the settings of test_gpu_lean.test_lean_proof_equals_oracle: at
    STEP42NS cm1_2ns is the arena just re-extended in place (in many batches)
    with the kept columns copied in"""
    from zkgpu.stark import GpuStark, MEM_LEAN
    if keep is None:
        monkeypatch.delenv("ZKGPU_LEAN_KEEP_COLS", raising=False)
    else:
        monkeypatch.setenv("ZKGPU_LEAN_KEEP_COLS", keep)
    inst = _inst(case)
    zkgpu.set_lde_batch_cols(batch)
    g = GpuStark(inst, mode=MEM_LEAN)
    try:
        assert g.memory_mode() == "lean"
        g.witness()
        _probed_proof_equals_oracle(g, inst, want[case], g.prove)
    finally:
        zkgpu.set_lde_batch_cols(0)
        g.close()


# ---------------------------------------------------------------- 3. streamed stage 1
@pytest.mark.parametrize("case", ["config4", "zkevm_shaped"])
def test_probe_streamed_stage1(zkgpu, want, monkeypatch, case):
    """prove_from_rows under the lean plan, cm1 arriving in 8-column batches
    (the smallest the call accepts): the same probe as set_cm1 + prove"""
    from zkgpu.stark import GpuStark, MEM_LEAN, MEM_RESIDENT
    monkeypatch.setenv("ZKGPU_STREAM_COLS", "8")
    monkeypatch.delenv("ZKGPU_STREAM_FAIL_BATCH", raising=False)
    monkeypatch.delenv("ZKGPU_LEAN_KEEP_COLS", raising=False)
    inst = _inst(case)
    r = GpuStark(inst, mode=MEM_RESIDENT)
    try:
        r.witness()
        rows = r.get_cm1()
    finally:
        r.close()
    g = GpuStark(inst, mode=MEM_LEAN)
    try:
        streamed = _probed_proof_equals_oracle(g, inst, want[case], lambda: g.prove_from_rows(rows))
        assert "STARK_STEP_1_STREAM" in g.timers()
        g.set_cm1(rows)
        assert g.prove() == want[case][1]
        zr.assert_same_probe(g.probe(), streamed)
    finally:
        g.close()


# ---------------------------------------------------------------- 4. blow-up 2
@pytest.mark.parametrize("mode", ["resident", "lean"])
def test_probe_blowup2(zkgpu, want, monkeypatch, mode):
    """the extended-domain shift reach at 1 << 2"""
    from zkgpu import ZkgpuError
    from zkgpu.stark import GpuStark, MEM_LEAN, MEM_RESIDENT
    monkeypatch.delenv("ZKGPU_LEAN_KEEP_COLS", raising=False)
    inst = _inst("blowup2")
    _, _, shifts = zr.program_sections(inst.programs["step42ns"])
    assert any(4 in s for s in shifts.values())
    try:
        g = GpuStark(inst, mode=MEM_LEAN if mode == "lean" else MEM_RESIDENT)
    except ZkgpuError as e:
        assert mode == "lean" and "lean memory plan does not apply" in str(e)
        return
    try:
        g.witness()
        _probed_proof_equals_oracle(g, inst, want["blowup2"], g.prove)
    finally:
        g.close()


# ---------------------------------------------------------------- 5. off means off
def test_probe_off_means_off(zkgpu, want):
    from zkgpu import ZkgpuError
    from zkgpu.stark import GpuStark, MEM_RESIDENT
    inst = _inst("config4")
    rn, re_ = _rows(inst)
    g = GpuStark(inst, mode=MEM_RESIDENT)
    zkgpu.prof_enable(True)
    try:
        g.witness()
        kernels, proofs = [], []

        def prove():
            zkgpu.prof_reset()
            proofs.append(g.prove_raw())
            kernels.append(zkgpu.prof_kernels())

        prove()
        assert g.probe_size() == (0, 0)
        with pytest.raises(ZkgpuError, match="no probe to read"):
            g.probe()
        g.probe_set(rn, re_)
        prove()
        n_recs, n_words = g.probe_size()
        assert n_recs == len(want["config4"][0]) and n_words > 0
        zr.assert_same_probe(g.probe(), want["config4"][0])
        g.probe_set([], [])
        assert g.probe_size() == (0, 0)
        prove()
        assert g.probe_size() == (0, 0)
        with pytest.raises(ZkgpuError, match="no probe to read"):
            g.probe()
        assert np.array_equal(proofs[0], proofs[1]) and np.array_equal(proofs[0], proofs[2])
        assert ["k_gather_rows" in k for k in kernels] == [False, True, False]
        assert sorted(set(kernels[1]) - {"k_gather_rows"}) == sorted(kernels[0]) == sorted(kernels[2])
        assert "ZKGPU_PROBE_READBACK" not in g.timers()
        # other rows: the next proof's probe has the new ones
        rn2, re2 = np.array([5, 3, 5], np.uint64), np.array([2047, 9], np.uint64)
        g.probe_set(rn2, re2)
        prove()
        got = g.probe()
        plan = zr.plan(inst, rn2, re2)
        assert [(p, a, s) for p, a, s, _, _ in got] == [(p, a, s) for p, a, s, _, _ in plan]
        for (_, _, _, r0, _), (_, _, _, _, r1) in zip(got, plan):
            assert np.array_equal(r0, r1)
        assert np.array_equal(proofs[3], proofs[0])
        assert zr.check_probe(inst, got, want["config4"][2]) == []
    finally:
        zkgpu.prof_enable(False)
        g.close()


# ---------------------------------------------------------------- 6. refusals
def test_probe_refusals(zkgpu):
    from zkgpu import ZkgpuError
    from zkgpu import synthetic as sy
    from zkgpu.stark import EXCHANGE, Comm, GpuStark, MEM_RESIDENT
    inst = _inst("config4")
    n, ne = 1 << inst.n_bits, 1 << inst.n_bits_ext
    g = GpuStark(inst, mode=MEM_RESIDENT)
    try:
        g.witness()
        with pytest.raises(ZkgpuError, match=r"row %d is outside the n domain" % n):
            g.probe_set([0, n], [0])
        with pytest.raises(ZkgpuError, match=r"row %d is outside the extended domain" % ne):
            g.probe_set([0], [ne])
        with pytest.raises(ZkgpuError, match="at most 4096 per domain"):
            g.probe_set(np.zeros(4097, np.uint64), [0])
        # a refusal leaves the probe off
        g.prove_raw()
        assert g.probe_size() == (0, 0)
        g.probe_set(np.zeros(4096, np.uint64), [1])  # repeats fold: one row
        g.prove_raw()
        n_recs, n_words = g.probe_size()
        assert n_recs > 0
        with pytest.raises(ZkgpuError, match="too small"):
            g.probe_read_raw(max_recs=n_recs - 1)
        with pytest.raises(ZkgpuError, match="too small"):
            g.probe_read_raw(max_words=n_words - 1)
    finally:
        g.close()
    # a stage-4 program that reads an n-domain section
    bad = copy.deepcopy(inst)
    p = bad.programs["step42ns"]
    a = p.o(sy.COL, sy.SEC_CM1_N, 0, 0)
    p.op(sy.ADD, p.o(sy.TMP1, 0, 0, 0), a, a)
    g = GpuStark(bad, mode=MEM_RESIDENT)
    try:
        with pytest.raises(ZkgpuError, match="step42ns reads section 0 of the other domain"):
            g.probe_set([0], [0])
    finally:
        g.close()

    class One:
        c = Comm(0, 1, None, EXCHANGE())

    g = GpuStark(inst, comm=One())
    try:
        with pytest.raises(ZkgpuError, match="probe_set is single-GPU only"):
            g.probe_set([0], [0])
    finally:
        g.close()
