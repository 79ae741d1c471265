"""zkgpu_lookup_misses_dev (csrc/h1h2.hip k_lookup_flag / k_lookup_emit over
the multiset table) against the pure-Python reference of tests/lookup_cases.py,
word for word: dim 1 and 3, sizes around the workgroup (256) and the
reduction's block (1024), ld = n + 3 with rows [n, ld) that would be misses if
read, every case run twice (the two results must be equal: nothing may depend
on which thread claims a slot), and every refusal."""
import functools

import numpy as np
import pytest

import lookup_cases as lc

pytestmark = pytest.mark.gpu

SENT = np.uint64(0xA5C3A5C3F00DFACE)
FILL = np.uint64(0x0123456789ABCDEF)  # rows [n, ld): a value no case holds
GUARD = 8


@functools.lru_cache(maxsize=None)
def table(n, dim):
    """the cases of one shape with their expected words (computed once)"""
    return [(c, lc.out_words(c.reference(), c.max_vals)) for c in lc.cases(n, dim)]


def image(col, ld):
    dim, n = col.shape
    img = np.full(dim * ld + GUARD, FILL, np.uint64)
    img[:dim * ld].reshape(dim, ld)[:, :n] = col
    return img


def run(zkgpu, case, dim):
    n = case.f.shape[1]
    ld = n + 3
    d_f = zkgpu.to_device(image(case.f, ld))
    d_t = d_f if case.same else zkgpu.to_device(image(case.t, ld))
    words = 2 + 2 * case.max_vals
    d_out = zkgpu.to_device(np.full(words + GUARD, SENT, np.uint64))
    zkgpu.lookup_misses_dev(d_out, d_f, ld, d_t, ld, n, dim, case.max_vals)
    zkgpu.synchronize()
    got = zkgpu.from_device(d_out)
    assert np.all(got[words:] == SENT), case.name  # nothing past the block
    return got[:words]


@pytest.mark.parametrize("dim", [1, 3])
@pytest.mark.parametrize("n", lc.SIZES)
def test_vs_reference(zkgpu, n, dim):
    for case, want in table(n, dim):
        first = run(zkgpu, case, dim)
        again = run(zkgpu, case, dim)
        print(case.name, first[:6], want[:6])
        assert np.array_equal(first, again), (case.name, "two runs differ")
        assert np.array_equal(first, want), (case.name, first[:10], want[:10])
        assert (int(first[0]), int(first[1])) == case.expect[:2], case.name  # what the construction promises


def test_host_wrapper(zkgpu):
    case = [c for c, _ in table(1000, 3) if c.name == "twenty_values"][0]
    assert zkgpu.lookup_misses(case.f, case.t, 16) == case.reference()
    case = [c for c, _ in table(257, 1) if c.name == "miss_row0_and_last"][0]
    assert zkgpu.lookup_misses(case.f[0], case.t[0]) == (2, 1, [(0, 2)])


def test_refusals(zkgpu):
    d_in = zkgpu.to_device(np.zeros(1024, np.uint64))
    d_out = zkgpu.to_device(np.full(2 + 2 * 4096 + GUARD, SENT, np.uint64))
    big = (1 << 28) + 1
    for args, message in (((d_out, d_in, 99, d_in, 100, 100, 1, 16), "lookup_misses: ld < n"),
                          ((d_out, d_in, 100, d_in, 99, 100, 1, 16), "lookup_misses: ld < n"),
                          ((d_out, d_in, 100, d_in, 100, 100, 2, 16), "lookup_misses: dim must be 1 or 3"),
                          ((d_out, d_in, 100, d_in, 100, 100, 0, 16), "lookup_misses: dim must be 1 or 3"),
                          ((d_out, d_in, 100, d_in, 100, 100, 3, 4097), "lookup_misses: max_vals 4097 > 4096"),
                          ((d_out, d_in, big, d_in, big, big, 1, 16), "lookup_misses: more than 2^28 rows"),
                          ((None, d_in, 100, d_in, 100, 100, 1, 16), "lookup_misses: null pointer"),
                          ((d_out, None, 100, d_in, 100, 100, 1, 16), "lookup_misses: null pointer"),
                          ((d_out, d_in, 100, None, 100, 100, 1, 16), "lookup_misses: null pointer")):
        with pytest.raises(zkgpu.ZkgpuError) as e:
            zkgpu.lookup_misses_dev(*args)
        assert str(e.value) == "zkgpu_lookup_misses_dev failed (-2): " + message
    zkgpu.synchronize()
    assert np.all(zkgpu.from_device(d_out) == SENT)  # nothing was queued
