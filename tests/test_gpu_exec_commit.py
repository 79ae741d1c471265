"""zkgpu_exec_commit_dev (csrc/exec.hip) against the reference loop restated
over Python ints (tests/exec_cases.py model, main.recursive1.cpp:343-394):
for every shared case the whole ld x n_cols block, written through a guard
pattern, equals the model word for word -- rows [0, n) of every column the
hand-off's, rows [n, ld) untouched -- for two witnesses on one handle;
zkgpu_exec_info gives the planner's counts; the argument refusals."""
import numpy as np
import pytest

import exec_cases as xc

pytestmark = pytest.mark.gpu

GUARD = 0xA5A5A5A5A5A5A5A5
CASES = xc.cases()


def _commit(zkgpu, ex, case, witness):
    import torch
    ld, n, nc = case["ld"], case["n"], case["n_cols"]
    d = zkgpu.to_device(np.full(ld * nc + 8, GUARD, np.uint64))
    ex.commit_dev(witness, d, ld, n)
    zkgpu.synchronize()
    torch.cuda.synchronize()
    out = zkgpu.from_device(d)
    assert (out[ld * nc:] == GUARD).all()
    return out[:ld * nc].reshape(nc, ld)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_commit_equals_the_model(zkgpu, case):
    ld, n, nc, sw = case["ld"], case["n"], case["n_cols"], case["size_witness"]
    ex = zkgpu.Exec(case["image"], sw, nc)
    try:
        lev, n_levels, segs = xc.schedule(case["image"], sw)
        info = ex.info()
        assert (info["n_adds"], info["n_smap"]) == (int(case["image"][0]), int(case["image"][1]))
        assert (info["n_levels"], info["n_launches"]) == (n_levels, segs + 1)
        # the tables (28 bytes an add, 4 a level, 4 a cell) and tmp, each rounded up to 256 bytes
        na = info["n_adds"]
        exact = 28 * na + 8 * (sw + na) + 4 * n_levels + 4 * info["n_smap"] * nc
        assert exact <= info["device_bytes"] <= exact + 8 * 256
        for seed in (1, 2):
            w = xc.witness_of(case, seed)
            want = np.full((nc, ld), GUARD, np.uint64)
            want[:, :n] = xc.model(w, case["image"], nc, n).T
            got = _commit(zkgpu, ex, case, w)
            bad = np.argwhere(got != want)
            assert bad.size == 0, (case["name"], seed, len(bad), bad[:5].tolist())
    finally:
        ex.close()


@pytest.mark.parametrize("tail,launches", [(256, 4), (1023, 4), (1024, 3)])
def test_tail_width_changes_the_launches_not_the_columns(zkgpu, tail, launches):
    """levels of T - 1, T, T + 1 adds under another tail width
    (zkgpu_exec_set_tail_width): grid launches where the level is wider"""
    case = next(c for c in CASES if c["name"].startswith("d_"))
    nc, sw = case["n_cols"], case["size_witness"]
    zkgpu.exec_set_tail_width(tail)
    try:
        ex = zkgpu.Exec(case["image"], sw, nc)
    finally:
        zkgpu.exec_set_tail_width(0)
    try:
        assert ex.info()["n_launches"] == launches == xc.schedule(case["image"], sw, tail)[2] + 1
        w = xc.witness_of(case, 3)
        got = _commit(zkgpu, ex, case, w)
        assert np.array_equal(got[:, :case["n"]], xc.model(w, case["image"], nc, case["n"]).T)
    finally:
        ex.close()
    with pytest.raises(zkgpu.ZkgpuError, match="tail width 1025 above 1024"):
        zkgpu.exec_set_tail_width(1025)
        try:
            zkgpu.Exec(case["image"], sw, nc)
        finally:
            zkgpu.exec_set_tail_width(0)


def test_refusals(zkgpu):
    from zkgpu import ZkgpuError
    case = CASES[0]
    sw, nc = case["size_witness"], case["n_cols"]
    with pytest.raises(ZkgpuError, match="the image has 20001 words, not 2 \\+ 4 x 2000 adds \\+ 1000 x 12 cells"):
        zkgpu.Exec(case["image"][:-1], sw, nc)
    bad = case["image"].copy()
    bad[2 + 4 * 9] = sw + 9
    with pytest.raises(ZkgpuError, match="add 9 reads slot 309, not below its own slot 309"):
        zkgpu.Exec(bad, sw, nc)
    ex = zkgpu.Exec(case["image"], sw, nc)
    try:
        d = zkgpu.to_device(np.full(1000 * nc, GUARD, np.uint64))
        w = xc.witness_of(case, 1)
        with pytest.raises(ZkgpuError, match="n = 999 rows, fewer than the sMap's 1000"):
            ex.commit_dev(w, d, 1000, 999)
        with pytest.raises(ZkgpuError, match="n = 1000 above ld = 999"):
            ex.commit_dev(w, d, 999, 1000)
        zkgpu.synchronize()
        assert (zkgpu.from_device(d) == GUARD).all()  # nothing was queued
    finally:
        ex.close()
