"""zkgpu_conn_breaks_dev (csrc/conn.hip k_conn_probe / k_conn_count /
k_conn_emit) against the pure-Python reference of tests/conn_cases.py, word for
word: shapes either side of the workgroup (256) and of the reduction's block
(1024), k n no power of two, ld = n + 3 with rows [n, ld) that would be findings
if read, the k columns permuted and scattered inside wider sections, a guard
past out, every case run twice (the two results must be equal), and every
refusal by its message with nothing queued."""
import functools

import numpy as np
import pytest

import conn_cases as cc

pytestmark = pytest.mark.gpu

SENT = np.uint64(0xA5C3A5C3F00DFACE)
FILL_A = np.uint64(0x0123456789ABCDEF)  # rows [n, ld) and the columns outside the lists
FILL_S = np.uint64(0)                   # (an S value that is no identity)
GUARD = 8
EXTRA = 3  # columns of a section that belong to no list


@functools.lru_cache(maxsize=None)
def table(n_bits, k):
    """the cases of one shape with their expected words (computed once)"""
    return [(c, cc.out_words(c.reference(), c.max_vals)) for c in cc.cases(n_bits, k)]


def image(cols, ld, where, fill):
    """a section of k + EXTRA columns with leading dimension ld, column i of cols at column where[i]"""
    k, n = cols.shape
    width = k + EXTRA
    img = np.full(width * ld + GUARD, fill, np.uint64)
    sec = img[:width * ld].reshape(width, ld)
    for i in range(k):
        sec[where[i], :n] = cols[i]
    return img


def run(zkgpu, case, lists):
    k, n = case.a.shape
    ld = n + 3
    a_cols, s_cols = lists
    d_a = zkgpu.to_device(image(case.a, ld, a_cols, FILL_A))
    d_s = zkgpu.to_device(image(case.s, ld, s_cols, FILL_S))
    words = 3 + 6 * case.max_vals
    d_out = zkgpu.to_device(np.full(words + GUARD, SENT, np.uint64))
    zkgpu.conn_breaks_dev(d_out, d_a, ld, a_cols, d_s, ld, s_cols, k, case.ks_arg, case.n_bits, case.max_vals)
    zkgpu.synchronize()
    got = zkgpu.from_device(d_out)
    assert np.all(got[words:] == SENT), case.name  # nothing past the block
    return got[:words]


@pytest.mark.parametrize("n_bits,k", cc.SHAPES)
def test_vs_reference(zkgpu, n_bits, k):
    rng = np.random.default_rng([3, n_bits, k])
    for case, want in table(n_bits, k):
        lists = tuple(rng.permutation(k + EXTRA)[:k].astype(np.uint32) for _ in range(2))
        first = run(zkgpu, case, lists)
        again = run(zkgpu, case, lists)
        print(case.name, first[:7], want[:7])
        assert np.array_equal(first, again), (case.name, "two runs differ")
        assert np.array_equal(first, want), (case.name, first[:11], want[:11])
        if case.expect is not None:
            assert tuple(int(x) for x in first[:3]) == case.expect, case.name  # what the construction promises


def test_default_column_lists_and_host_wrapper(zkgpu):
    case = [c for c, _ in table(8, 3) if c.name == "one_off_middle"][0]
    counts, breaks, foreign = zkgpu.conn_breaks(case.a, case.s)
    assert (counts, breaks, foreign) == case.reference() and counts == (2, 0, 0)
    case = [c for c, _ in table(5, 2) if c.name == "own_ks_mismatch"][0]
    assert zkgpu.conn_breaks(case.a, case.s, ks=case.ks, max_vals=4) == cc.reference(case.a, case.s, case.ks, 5, 4)
    case = [c for c, _ in table(5, 3) if c.name == "foreign_coset_at_0"][0]
    assert zkgpu.conn_breaks(case.a, case.s, max_vals=2) == cc.reference(case.a, case.s, case.ks, 5, 2)


def test_refusals(zkgpu):
    d_in = zkgpu.to_device(np.zeros(4096, np.uint64))
    d_out = zkgpu.to_device(np.full(3 + 6 * 4096 + GUARD, SENT, np.uint64))
    w3 = cc.omega(3)
    M = "conn_breaks: "
    # (out, a, a_ld, a_cols, s, s_ld, s_cols, k, ks, n_bits, max_vals)
    for args, message in (((d_out, d_in, 7, None, d_in, 8, None, 2, None, 3, 16), M + "ld < n"),
                          ((d_out, d_in, 8, None, d_in, 7, None, 2, None, 3, 16), M + "ld < n"),
                          ((d_out, d_in, 8, None, d_in, 8, None, 0, None, 3, 16), M + "k = 0 not in 1 .. 64"),
                          ((d_out, d_in, 8, None, d_in, 8, None, 65, None, 3, 16), M + "k = 65 not in 1 .. 64"),
                          ((d_out, d_in, 1 << 28, None, d_in, 1 << 28, None, 9, None, 28, 16),
                           M + "more than 2^31 cells"),
                          ((d_out, d_in, 1 << 29, None, d_in, 1 << 29, None, 1, None, 29, 16),
                           M + "more than 2^28 rows"),
                          ((d_out, d_in, 8, None, d_in, 8, None, 2, None, 3, 4097), M + "max_vals 4097 > 4096"),
                          ((d_out, d_in, 8, [0, 1, 0], d_in, 8, None, 3, None, 3, 16),
                           M + "column 0 repeated in a_cols"),
                          ((d_out, d_in, 8, None, d_in, 8, [2, 5, 5], 3, None, 3, 16),
                           M + "column 5 repeated in s_cols"),
                          ((d_out, d_in, 8, None, d_in, 8, None, 2, [1, 0], 3, 16), M + "ks[1] is zero"),
                          ((d_out, d_in, 8, None, d_in, 8, None, 2, [5, cc.P], 3, 16), M + "ks[1] is zero"),
                          ((d_out, d_in, 8, None, d_in, 8, None, 3, [3, 5, 3 * w3 % cc.P], 3, 16),
                           M + "the cosets of ks[0] and ks[2] collide"),
                          ((None, d_in, 8, None, d_in, 8, None, 2, None, 3, 16), M + "null pointer"),
                          ((d_out, None, 8, None, d_in, 8, None, 2, None, 3, 16), M + "null pointer"),
                          ((d_out, d_in, 8, None, None, 8, None, 2, None, 3, 16), M + "null pointer")):
        with pytest.raises(zkgpu.ZkgpuError) as e:
            zkgpu.conn_breaks_dev(*args)
        assert str(e.value) == "zkgpu_conn_breaks_dev failed (-2): " + message
    zkgpu.synchronize()
    assert np.all(zkgpu.from_device(d_out) == SENT)  # nothing was queued
