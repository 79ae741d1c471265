"""The Poseidon partial rounds as three-round power blocks, on the GPU.

csrc/poseidon_perm.hpp partial_rounds_pow3 replaces the 64-bit-coefficient
block form in every thread-per-state kernel.  Here: its two-accumulator
reduction (Dot2::fin, zkgpu_gl_field_selftest_rb_dev op 12) on the inputs
tests/psb3_cases.py builds for each of its carries, in all 64 lanes of a wave
and in one lane of an ordinary wave, against Python integers; the full and the
four-lane permutation on edge, constructed and random states against the
oracle (PoseidonGoldilocks::hash_full_result restated); leaf digests and whole
trees against the oracle's merkletree for one, several and ragged sponge
blocks in both leaf layouts, and trees large enough that the thread-per-node,
the lane-parallel and the tail level kernels all run.
"""
import random

import numpy as np
import pytest

import psb3_cases as pc

P = pc.P


# ------------------------------------------------------------------ Dot2::fin
def _waves(cases, rng):
    """each case in all 64 lanes of a wave, then in one lane (0, 63, a random one in turn) of a
    wave of ordinary accumulators"""
    rows = []
    for k, c in enumerate(cases):
        rows += [c] * 64
        lane = (0, 63, rng.randrange(1, 63))[k % 3]
        for i in range(64):
            rows.append(c if i == lane else (rng.randint(0, pc.ACC_MAX), rng.randint(0, pc.ACC_MAX)))
    return rows


def _run_fin(zkgpu, rows):
    import torch
    n = len(rows)
    a = np.array([r[0] for r in rows], dtype=np.uint64)
    b = np.array([r[1] for r in rows], dtype=np.uint64)
    out = torch.zeros(n, dtype=torch.int64, device="cuda:0")
    zkgpu.field_selftest_rb_dev(out, zkgpu.to_device(a), zkgpu.to_device(b), None, n, pc.DOT2FIN, 0)
    torch.cuda.synchronize()
    got = zkgpu.from_device(out)
    bad = [i for i in range(n) if int(got[i]) != pc.fin_ref(*rows[i])]
    assert not bad, [(i, hex(rows[i][0]), hex(rows[i][1]), hex(int(got[i]))) for i in bad[:5]]


@pytest.mark.gpu
def test_dot2_fin_constructed(zkgpu):
    rng = random.Random(212)
    _run_fin(zkgpu, _waves(pc.fin_cases(rng), rng))


@pytest.mark.gpu
def test_dot2_fin_random(zkgpu):
    rng = random.Random(213)
    rows = [(rng.randint(0, pc.ACC_MAX), rng.randint(0, pc.ACC_MAX)) for _ in range(1 << 15)]
    rows += [(rng.randint(0, pc.M64), rng.randint(0, pc.WIDE)) for _ in range(1 << 15)]
    _run_fin(zkgpu, rows)


# ------------------------------------------------------------------ the permutation
def _perm_states(n):
    st = pc.edge_states()
    for k in range(8):  # the first partial round's S-box input is 0 / p - 1
        st.append(pc.state_with_lane0_after_full4(0, 100 + k))
        st.append(pc.state_with_lane0_after_full4(P - 1, 200 + k))
    x = np.array(st + pc.random_states(n - len(st), 99), dtype=np.uint64)
    x[n // 2:n // 2 + 8, 8:] = 0  # zero capacity: the four-lane kernel's constant round 0 (where it applies)
    return x


@pytest.fixture(scope="module")
def perm_case(oracle):
    n = 4096
    x = _perm_states(n)
    return x, np.stack([oracle.poseidon_full(x[i]) for i in range(n)])


@pytest.mark.gpu
@pytest.mark.parametrize("full", [True, False], ids=["full", "four"])
def test_poseidon_batch_vs_oracle(zkgpu, perm_case, full):
    import torch
    x, exp = perm_case
    n = x.shape[0]
    out = torch.zeros((n, 12 if full else 4), dtype=torch.int64, device="cuda:0")
    zkgpu.poseidon_batch_dev(out, zkgpu.to_device(x), n, full)
    torch.cuda.synchronize()
    assert np.array_equal(zkgpu.from_device(out), exp if full else exp[:, :4])


# ------------------------------------------------------------------ leaves and trees
WIDTHS = [1, 4, 5, 8, 9, 26, 27, 100]


def _rows(nrows, ncols, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, P, size=(nrows, ncols), dtype=np.uint64)
    x[0] = 0
    x[1] = P - 1
    return x


def _tree(zkgpu, x, rows_major):
    import torch
    nrows, ncols = x.shape
    nodes = torch.zeros(zkgpu.merkle_num_elements(nrows), dtype=torch.int64, device="cuda:0")
    if rows_major:
        zkgpu.merkletree_rows_dev(nodes, zkgpu.to_device(x), ncols, nrows)
    else:
        zkgpu.merkletree_dev(nodes, zkgpu.to_device(np.ascontiguousarray(x.T)), nrows, ncols, nrows)
    torch.cuda.synchronize()
    return zkgpu.from_device(nodes)


@pytest.mark.gpu
@pytest.mark.parametrize("rows_major", [False, True], ids=["cols", "rows"])
@pytest.mark.parametrize("ncols", WIDTHS)
@pytest.mark.parametrize("bits", [8, 10])
def test_leaves_and_tree_vs_oracle(oracle, zkgpu, bits, ncols, rows_major):
    """leaf digests (the first 4 * nrows node words) and every level above them"""
    nrows = 1 << bits
    x = _rows(nrows, ncols, 3000 + 16 * bits + ncols)
    got, exp = _tree(zkgpu, x, rows_major), oracle.merkletree(x)
    assert np.array_equal(got[:4 * nrows], exp[:4 * nrows]), "leaf digests"
    assert np.array_equal(exp[4:8], oracle.linear_hash(x[1]))
    assert np.array_equal(got, exp)


@pytest.mark.gpu
def test_tree_2p16_vs_oracle(oracle, zkgpu):
    """2^16 rows of 9 columns: thread-per-row leaves, lane-parallel levels from 2^15 nodes down
    and the tail kernel"""
    x = _rows(1 << 16, 9, 61)
    assert np.array_equal(_tree(zkgpu, x, False), oracle.merkletree(x))


@pytest.mark.gpu
def test_tree_2p17_thread_level_vs_oracle(oracle, zkgpu):
    """the thread-per-node level kernel takes over above 2^15 nodes per level: the first level
    of a 2^17-leaf tree (width 4: the leaves are the rows themselves), then the lane-parallel
    levels and the tail"""
    x = _rows(1 << 17, 4, 62)
    assert np.array_equal(_tree(zkgpu, x, False), oracle.merkletree(x))
