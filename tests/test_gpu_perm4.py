"""The borrow of gl_reduce128_rb at its boundary, the four-lane permutation
and the sponge / tree kernels that use it.

gl_reduce128_rb (csrc/gl_rb.hpp) takes the borrow of lo - hh from a 32-bit
subtract-with-borrow chain; the rare correction runs when some lane of the
wave has lo < hh.  The cases here sit on that boundary: lo == hh (no borrow),
lo == hh - 1 (borrow), a borrow of the low word that the high word absorbs,
and the extreme words.  They go through zkgpu_gl_field_selftest_rb_dev op 3
(lo = a, hi = b) and, as products with those 128-bit values, op 2, in every
lane of a wave and in one lane of an otherwise ordinary wave, against Python
integers.  test_borrow_cases_cpu checks the constructions without a GPU.

perm_fast4 (csrc/poseidon_perm.hpp) computes only lanes 0..3 of the last
linear layer, and for a zero capacity replaces round 0 of lanes 8..11 by
constants: checked against the full permutation, and through the leaf and
tree kernels against the oracle (linear_hash / merkletree: the reference's
PoseidonGoldilocks::linear_hash and merkletree).
"""
import random

import numpy as np
import pytest

import rb_cases as rc

P, M = rc.P, rc.M64
W32 = 0xFFFFFFFF


# ------------------------------------------------------------------ borrow boundary
def _red_cases():
    """(name, lo, hi, borrows) for op 3"""
    out = []
    for hh, hl in [(1, 0), (5, 0x1234), (W32, W32), (0x80000000, 7)]:
        hi = (hh << 32) | hl
        out.append(("eq", hh, hi, False))            # l1 = 0, l0 = hh
        out.append(("below", hh - 1, hi, True))      # l1 = 0, l0 = hh - 1
    for hl in (0, 1, W32):
        out.append(("absorbed", 1 << 32, (W32 << 32) | hl, False))  # l1 = 1, l0 = 0, hh = 2^32 - 1
    out.append(("zero", 0, 0, False))
    out.append(("himax_lo0", 0, M, True))
    out.append(("himax_lo_below", (1 << 32) - 2, M, True))
    out.append(("himax_lomax", M, M, False))
    return out


def _mul_cases():
    """(name, a, b, lo, hi, borrows): products whose 128-bit value sits on the
    boundary.  hh (2^96 + 1) = hh (2^32 + 1) p gives lo = hh, hi = hh 2^32;
    (2^64 - 1)(2^64 - s) = (2^64 - s - 1) 2^64 + s gives hh = 2^32 - 1, lo = s
    for s < 2^32; (2^64 - 2)(2^64 - 2^31) has lo = 2^32, hh = 2^32 - 1."""
    out = []
    for hh in (1, 0x9E3779B9, W32):
        out.append(("eq", P, hh * ((1 << 32) + 1), hh, hh << 32, False))
    out.append(("eq", M, (1 << 64) - W32, W32, ((1 << 64) - W32 - 1), False))
    out.append(("below", M, (1 << 64) - (W32 - 1), W32 - 1, (1 << 64) - W32, True))
    out.append(("absorbed", M - 1, (1 << 64) - (1 << 31), 1 << 32, (1 << 64) - (1 << 31) - 2, False))
    out.append(("zero", 0, 0x123456789ABCDEF, 0, 0, False))
    out.append(("max", M, M, 1, M - 1, True))
    return out


def test_borrow_cases_cpu():
    """the constructed cases are what they claim, in Python integers"""
    seen = set()
    for name, lo, hi, br in _red_cases():
        assert 0 <= lo <= M and 0 <= hi <= M
        assert rc.taken_red128(lo, hi) == br, name
        hh, l0, l1 = hi >> 32, lo & W32, lo >> 32
        if name == "eq":
            assert l1 == 0 and l0 == hh
        if name == "below":
            assert l1 == 0 and l0 == hh - 1
        if name == "absorbed":
            assert l1 == 1 and l0 == 0 and hh == W32 and l0 < hh  # the low word borrows, the pair does not
        seen.add(name)
    assert seen == {"eq", "below", "absorbed", "zero", "himax_lo0", "himax_lo_below", "himax_lomax"}
    for name, a, b, lo, hi, br in _mul_cases():
        assert 0 <= a <= M and 0 <= b <= M
        assert a * b == (hi << 64) + lo, name
        assert rc.taken_mul(a, b) == br == rc.taken_red128(lo, hi), name
        hh, l0, l1 = hi >> 32, lo & W32, lo >> 32
        if name == "eq":
            assert l1 == 0 and l0 == hh
        if name == "below":
            assert l1 == 0 and l0 == hh - 1
        if name == "absorbed":
            assert l1 == 1 and l0 == 0 and hh == W32
    # the reference value of both ops for a boundary case
    assert rc.ref(rc.RED128, 5, (5 << 32)) == (5 + (5 << 96)) % P == 0


def _waves(cases, rng):
    """each case in all 64 lanes of a wave, then in one lane (0, 63, a random
    one in turn) of a wave of ordinary values"""
    rows = []
    for k, c in enumerate(cases):
        rows += [c] * 64
        lane = (0, 63, rng.randrange(1, 63))[k % 3]
        for i in range(64):
            rows.append(c if i == lane else tuple(rc.ordinary(rng, 2)))
    return rows


def _run(zkgpu, op, rows):
    import torch
    n = len(rows)
    a = np.array([r[0] for r in rows], dtype=np.uint64)
    b = np.array([r[1] for r in rows], dtype=np.uint64)
    out = torch.zeros(n, dtype=torch.int64, device="cuda:0")
    zkgpu.field_selftest_rb_dev(out, zkgpu.to_device(a), zkgpu.to_device(b), zkgpu.to_device(np.zeros(n, np.uint64)),
                                n, op, 0)
    torch.cuda.synchronize()
    got = zkgpu.from_device(out)
    bad = [i for i in range(n) if int(got[i]) != rc.ref(op, rows[i][0], rows[i][1])]
    assert not bad, [(i, hex(rows[i][0]), hex(rows[i][1]), hex(int(got[i]))) for i in bad[:5]]


@pytest.mark.gpu
def test_reduce128_borrow_boundary(zkgpu):
    rng = random.Random(128)
    _run(zkgpu, rc.RED128, _waves([(lo, hi) for _, lo, hi, _ in _red_cases()], rng))


@pytest.mark.gpu
def test_mul_borrow_boundary(zkgpu):
    rng = random.Random(2)
    _run(zkgpu, rc.MUL, _waves([(a, b) for _, a, b, _, _, _ in _mul_cases()], rng))


@pytest.mark.gpu
@pytest.mark.parametrize("op", [rc.RED128, rc.MUL], ids=["reduce128", "mul"])
def test_borrow_random_pairs(zkgpu, op):
    rng = random.Random(300 + op)
    _run(zkgpu, op, [(rng.randint(0, M), rng.randint(0, M)) for _ in range(1 << 16)])


# ------------------------------------------------------------------ four-lane permutation
def _states(n):
    rng = np.random.default_rng(412)
    x = rng.integers(0, P, size=(n, 12), dtype=np.uint64)
    x[0] = 0
    x[1] = P - 1
    x[2:n // 2, 8:] = 0                 # zero capacity (a tree node, a first block)
    x[3, :8] = P - 1
    x[4, :8] = 0
    x[4, 8:] = P - 1
    x[n // 2:n // 2 + 64] = rng.integers(P, 1 << 64, size=(64, 12), dtype=np.uint64, endpoint=False)  # lazy words
    return x


@pytest.mark.gpu
def test_perm4_vs_full(oracle, zkgpu):
    import torch
    n = 4096
    x = _states(n)
    din = zkgpu.to_device(x)
    full = torch.zeros((n, 12), dtype=torch.int64, device="cuda:0")
    four = torch.zeros((n, 4), dtype=torch.int64, device="cuda:0")
    zkgpu.poseidon_batch_dev(full, din, n, True)
    zkgpu.poseidon_batch_dev(four, din, n, False)
    torch.cuda.synchronize()
    full, four = zkgpu.from_device(full), zkgpu.from_device(four)
    assert np.array_equal(four, full[:, :4])
    for i in (0, 1, 2, 3, 4, n - 1):
        assert np.array_equal(four[i], oracle.poseidon_full(x[i])[:4])


# ------------------------------------------------------------------ leaves and trees
WIDTHS = [1, 4, 5, 8, 9, 12, 16, 17, 26, 27, 100]


def _rows(nrows, ncols, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, P, size=(nrows, ncols), dtype=np.uint64)
    x[0] = 0          # all-zero row: every product of its first block sees zero words
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
def test_leaf_digests_vs_linear_hash(oracle, zkgpu, ncols, rows_major):
    nrows = 1 << 8
    x = _rows(nrows, ncols, 1000 + ncols)
    got = _tree(zkgpu, x, rows_major)[:4 * nrows].reshape(nrows, 4)
    exp = np.stack([oracle.linear_hash(x[i]) for i in range(nrows)])
    assert np.array_equal(got, exp)


@pytest.mark.gpu
def test_leaf_digests_rows_kernel_per_thread(oracle, zkgpu):
    """above 2^15 rows the row-major source takes the one-thread-per-row
    kernel (below: 16 lanes per row); two blocks, the second padded"""
    nrows, ncols = (1 << 15) + 256, 9
    x = _rows(nrows, ncols, 77)
    # leaves only matter here: a tree needs a power of two, so hash 2^16 rows
    # whose tail repeats the head
    xx = np.concatenate([x, x[:(1 << 16) - nrows]])
    got = _tree(zkgpu, xx, True)[:4 * nrows].reshape(nrows, 4)
    exp = oracle.merkletree(xx)[:4 * nrows].reshape(nrows, 4)
    assert np.array_equal(got, exp)
    assert np.array_equal(exp[5], oracle.linear_hash(x[5]))


@pytest.mark.gpu
@pytest.mark.parametrize("rows_major", [False, True], ids=["cols", "rows"])
def test_tree_2p10_vs_oracle(oracle, zkgpu, rows_major):
    """every level of a 2^10-leaf tree: the lane-parallel levels and the tail
    kernel"""
    x = _rows(1 << 10, 12, 5)
    assert np.array_equal(_tree(zkgpu, x, rows_major), oracle.merkletree(x))


@pytest.mark.gpu
def test_tree_2p17_thread_level_vs_oracle(oracle, zkgpu):
    """the first level of a 2^17-leaf tree (2^16 nodes) runs the
    one-thread-per-node kernel, whose capacity lanes are the round-0 constants;
    width 4: the leaves are the rows themselves"""
    x = _rows(1 << 17, 4, 6)
    assert np.array_equal(_tree(zkgpu, x, False), oracle.merkletree(x))
