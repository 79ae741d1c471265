"""zkgpu_multiset_diff_dev (csrc/h1h2.hip k_ms_insert / k_ms_flag / k_ms_emit)
against the pure-Python reference of tests/multiset_cases.py, word for word:
dim 1 and 3, sizes around the workgroup (256), the reduction's block (1024)
and 2^16, a_ld != b_ld with rows [n, ld) that would create mismatches if read,
every case run twice (the two results must be equal: nothing may depend on
which thread claims a slot)."""
import functools

import numpy as np
import pytest

import multiset_cases as mc

pytestmark = pytest.mark.gpu

SENT = np.uint64(0xA5C3A5C3F00DFACE)
FILL = np.uint64(0x0123456789ABCDEF)  # rows [n, ld): a value no case holds
GUARD = 8


@functools.lru_cache(maxsize=None)
def table(n, dim):
    """the cases of one shape with their expected words (computed once)"""
    return [(c, mc.out_words(c.reference(), c.max_vals)) for c in mc.cases(n, dim)]


def image(col, ld):
    dim, n = col.shape
    img = np.full(dim * ld + GUARD, FILL, np.uint64)
    img[:dim * ld].reshape(dim, ld)[:, :n] = col
    return img


def run(zkgpu, case, dim):
    n = case.a.shape[1]
    a_ld, b_ld = n + 5, n + 11
    d_a = zkgpu.to_device(image(case.a, a_ld))
    d_b = d_a if case.same else zkgpu.to_device(image(case.b, b_ld))
    if case.same:
        b_ld = a_ld
    words = 2 * (1 + 3 * case.max_vals)
    d_out = zkgpu.to_device(np.full(words + GUARD, SENT, np.uint64))
    zkgpu.multiset_diff_dev(d_out, d_a, a_ld, d_b, b_ld, n, dim, case.max_vals)
    zkgpu.synchronize()
    got = zkgpu.from_device(d_out)
    assert np.all(got[words:] == SENT), case.name  # nothing past the two blocks
    return got[:words]


@pytest.mark.parametrize("dim", [1, 3])
@pytest.mark.parametrize("n", mc.SIZES)
def test_vs_reference(zkgpu, n, dim):
    for case, want in table(n, dim):
        first = run(zkgpu, case, dim)
        again = run(zkgpu, case, dim)
        assert np.array_equal(first, again), (case.name, "two runs differ")
        assert np.array_equal(first, want), (case.name, first[:10], want[:10])
        if case.expect is not None:  # what the construction promises
            n_a, la, n_b, lb = case.expect
            assert (int(first[0]), int(first[1 + 3 * case.max_vals])) == (n_a, n_b), case.name


def test_three_against_two_is_in_both_blocks(zkgpu):
    case = [c for c, _ in table(1000, 3) if c.name == "three_against_two"][0]
    got = run(zkgpu, case, 3)
    a, b = mc.tuples(case.a), mc.tuples(case.b)
    v = [x for x in set(a) if a.count(x) == 3][0]
    assert got[0] == 1 and tuple(got[1:4]) == (a.index(v), 3, 2)  # the lowest occurrence in a
    blk = got[1 + 3 * 16:]
    assert blk[0] == 2 and (b.index(v), 3, 2) in [tuple(int(x) for x in blk[1 + 3 * k:4 + 3 * k]) for k in range(2)]


def test_empty_columns_write_zero_counts(zkgpu):
    d_in = zkgpu.to_device(np.full(64, FILL, np.uint64))
    for dim in (1, 3):
        for mv in (0, 16):
            words = 2 * (1 + 3 * mv)
            d_out = zkgpu.to_device(np.full(words + GUARD, SENT, np.uint64))
            zkgpu.multiset_diff_dev(d_out, d_in, 8, d_in, 8, 0, dim, mv)
            zkgpu.synchronize()
            want = np.concatenate([mc.out_words((0, [], 0, []), mv), np.full(GUARD, SENT, np.uint64)])
            assert np.array_equal(zkgpu.from_device(d_out), want)


def test_refusals(zkgpu):
    d_in = zkgpu.to_device(np.zeros(1024, np.uint64))
    d_out = zkgpu.to_device(np.full(2 * (1 + 3 * 4096) + GUARD, SENT, np.uint64))
    big = (1 << 28) + 1
    for args, message in (((d_out, d_in, 99, d_in, 100, 100, 1, 16), "multiset_diff: ld < n"),
                          ((d_out, d_in, 100, d_in, 99, 100, 1, 16), "multiset_diff: ld < n"),
                          ((d_out, d_in, 100, d_in, 100, 100, 2, 16), "multiset_diff: dim must be 1 or 3"),
                          ((d_out, d_in, 100, d_in, 100, 100, 0, 16), "multiset_diff: dim must be 1 or 3"),
                          ((d_out, d_in, 100, d_in, 100, 100, 3, 4097), "multiset_diff: max_vals 4097 > 4096"),
                          ((d_out, d_in, big, d_in, big, big, 1, 16), "multiset_diff: more than 2^28 rows"),
                          ((None, d_in, 100, d_in, 100, 100, 1, 16), "multiset_diff: null pointer"),
                          ((d_out, None, 100, d_in, 100, 100, 1, 16), "multiset_diff: null pointer"),
                          ((d_out, d_in, 100, None, 100, 100, 1, 16), "multiset_diff: null pointer")):
        with pytest.raises(zkgpu.ZkgpuError) as e:
            zkgpu.multiset_diff_dev(*args)
        assert str(e.value) == "zkgpu_multiset_diff_dev failed (-2): " + message
    zkgpu.synchronize()
    assert np.all(zkgpu.from_device(d_out) == SENT)  # nothing was queued
