"""The stage primitives on the GPU at ragged sizes, strides and lazy words.

csrc/stark.hip's grand product (k_z_ratio / k_z_totals / k_z_apply),
k_ext_powers, k_qsplit, k_cols3_to_interleaved, k_copy_rows, k_rand_cols and
csrc/ntt.hip's transposes, through their C-ABI entry points, at the sizes of
tests/stage_cases.py (checked on the CPU by tests/test_stage_cases.py).
Every comparison is bit-exact: the expected value is the oracle on the inputs
reduced mod p, and the Python-integer reference as well up to 2048 rows.
Every output buffer starts as a sentinel word; whole buffers are compared, so
the rows in [n, ld), the columns not named and a guard past the end must
still hold it.  Input buffers carry another filler in their rows [n, ld),
which a kernel reading past n would fold into its result.
"""
import functools

import numpy as np
import pytest

import stage_cases as sc

pytestmark = pytest.mark.gpu

P = sc.P
SENT = np.uint64(0xA5C3A5C3F00DFACE)  # what no call may overwrite
FILL = np.uint64(0x0123456789ABCDEF)  # input rows no call may read
GUARD = 64


def image(ncols, ld):
    """host image of an untouched output buffer, and its (ncols, ld) view"""
    img = np.full(ncols * ld + GUARD, SENT, dtype=np.uint64)
    return img, img[:ncols * ld].reshape(ncols, ld)


def dev_out(zkgpu, ncols, ld):
    return zkgpu.to_device(image(ncols, ld)[0])


def dev_in(zkgpu, cols, ld):
    """(ncols, n) columns at leading dimension ld, FILL elsewhere"""
    ncols, n = cols.shape
    img = np.full(ncols * ld + GUARD, FILL, dtype=np.uint64)
    img[:ncols * ld].reshape(ncols, ld)[:, :n] = cols
    return zkgpu.to_device(img)


def fetch(zkgpu, t):
    zkgpu.synchronize()
    return zkgpu.from_device(t)


def expect_cols(ncols, ld, cols, at=None):
    """the image with `cols` (k, n) in rows [0, n) of columns `at` (default 0..k-1)"""
    img, v = image(ncols, ld)
    for k, col in enumerate(cols):
        v[k if at is None else at[k], :len(col)] = col
    return img


# ------------------------------------------------------------------ grand product
@functools.lru_cache(maxsize=None)
def z_case(n):
    return sc.ZCase(n)


@functools.lru_cache(maxsize=None)
def z_expected(oracle, n, which):
    """(z columns, closes) of the case's product with denominator `which`; computed once"""
    case = z_case(n)
    z, total, closes = sc.oracle_calculate_z(oracle, case.num, case.dens()[which])
    if n <= sc.PY_REF_MAX:
        zr, tr = sc.ref_calculate_z(sc.rows3(case.num), sc.rows3(case.dens()[which]))
        assert np.array_equal(sc.cols3(zr), z) and tr == total
    z.setflags(write=False)
    return z, closes


def z_upload(zkgpu, case, which):
    _, num_ld, den_ld = sc.z_lds(case.n)
    num = case.num_lazy if which == "lazy" else case.num
    return dev_in(zkgpu, num, num_ld), dev_in(zkgpu, case.dens()[which], den_ld)


@pytest.mark.parametrize("n", sc.Z_N)
def test_calculate_z_ragged(oracle, zkgpu, n):
    """three different leading dimensions above n; canonical and lazy inputs
    give the same canonical z and both close; one denominator word changed in
    the last row, or in row 0, is reported"""
    case = z_case(n)
    z_ld, num_ld, den_ld = sc.z_lds(n)
    got = {}
    for which in ("closing", "lazy", "bad_last", "bad_first"):
        dnum, dden = z_upload(zkgpu, case, which)
        dz = dev_out(zkgpu, 3, z_ld)
        closes = zkgpu.calculate_z_dev(dz, z_ld, dnum, num_ld, dden, den_ld, n)
        z, exp_closes = z_expected(oracle, n, which)
        got[which] = fetch(zkgpu, dz)
        print("n=%d %s: closes %s (expected %s)" % (n, which, closes, exp_closes))
        assert exp_closes == (which in ("closing", "lazy"))
        assert closes == exp_closes, which
        assert np.array_equal(got[which], expect_cols(3, z_ld, z)), which
    assert np.array_equal(got["closing"], got["lazy"])
    assert got["lazy"][:3 * z_ld].reshape(3, z_ld)[:, :n].max() < P


@pytest.mark.parametrize("n", sc.Z_BLOCK_N)
def test_calculate_z_block_lazy_z0(oracle, zkgpu, n):
    """a z0 that is neither the unit nor canonical, over a product that does
    not close: z = z0 * running product, total = z0 * prod, both canonical"""
    case = sc.ZBlockCase(n)
    z_ld, num_ld, den_ld = sc.z_lds(n)
    z, total, _ = sc.oracle_calculate_z(oracle, case.num, case.den, sc.Z0_LAZY)
    if n <= sc.PY_REF_MAX:
        zr, tr = sc.ref_calculate_z(sc.rows3(case.num), sc.rows3(case.den), sc.Z0_LAZY)
        assert np.array_equal(sc.cols3(zr), z) and tr == total
    dz = dev_out(zkgpu, 3, z_ld)
    tot = zkgpu.calculate_z_block_dev(dz, z_ld, dev_in(zkgpu, case.num, num_ld), num_ld,
                                      dev_in(zkgpu, case.den, den_ld), den_ld, n, sc.Z0_LAZY)
    print("n=%d total %s expected %s" % (n, [int(v) for v in tot], list(total)))
    assert tuple(int(v) for v in tot) == total
    assert np.array_equal(fetch(zkgpu, dz), expect_cols(3, z_ld, z))


def test_calculate_z_block_empty(zkgpu):
    """n = 0: the total is z0 mod p and nothing is touched"""
    dz = dev_out(zkgpu, 3, 4)
    d = dev_in(zkgpu, np.ones((3, 1), np.uint64), 4)
    assert [int(v) for v in zkgpu.calculate_z_block_dev(dz, 4, d, 4, d, 4, 0, sc.Z0_LAZY)] == [5, 2**32 - 2, 0]
    assert np.array_equal(fetch(zkgpu, dz), image(3, 4)[0])


def _many(oracle, zkgpu, n):
    """five requests over one n, each with its own leading dimensions: a
    failing product between closing ones, a lazy one, one failing in row 0"""
    case = z_case(n)
    order = ["closing", "bad_last", "lazy", "bad_first", "closing"]
    reqs, outs = [], []
    for k, which in enumerate(order):
        z_ld, num_ld, den_ld = (ld + 5 * k for ld in sc.z_lds(n))
        num = case.num_lazy if which == "lazy" else case.num
        dz = dev_out(zkgpu, 3, z_ld)
        outs.append((dz, z_ld))
        reqs.append((dz, z_ld, dev_in(zkgpu, num, num_ld), num_ld, dev_in(zkgpu, case.dens()[which], den_ld), den_ld))
    closes = zkgpu.calculate_z_many_dev(reqs, n)
    print("n=%d closes %s" % (n, closes))
    assert closes == [True, False, True, False, True]
    for which, (dz, z_ld) in zip(order, outs):
        assert np.array_equal(fetch(zkgpu, dz), expect_cols(3, z_ld, z_expected(oracle, n, which)[0])), which


@pytest.mark.parametrize("n", sc.Z_MANY_N)
def test_calculate_z_many(oracle, zkgpu, n):
    _many(oracle, zkgpu, n)


def test_calculate_z_many_stale_scratch(oracle, zkgpu):
    """the grow-only scratch is shared by the requests and across calls: a
    long call, then short ones whose tile totals and prefixes lie where the
    long call left its ratios"""
    for n in sc.Z_STALE_SEQUENCE:
        _many(oracle, zkgpu, n)
    n = sc.Z_STALE_SEQUENCE[1]
    case = z_case(n)
    z_ld, num_ld, den_ld = sc.z_lds(n)
    dnum, dden = z_upload(zkgpu, case, "bad_first")
    dz = dev_out(zkgpu, 3, z_ld)
    assert not zkgpu.calculate_z_dev(dz, z_ld, dnum, num_ld, dden, den_ld, n)
    assert np.array_equal(fetch(zkgpu, dz), expect_cols(3, z_ld, z_expected(oracle, n, "bad_first")[0]))


def test_calculate_z_refusals(zkgpu):
    n = 8
    d = dev_in(zkgpu, np.ones((3, n), np.uint64), n)
    dz = dev_out(zkgpu, 3, n)
    for lds in ((n - 1, n, n), (n, n - 1, n), (n, n, n - 1)):
        with pytest.raises(zkgpu.ZkgpuError, match="ld < n"):
            zkgpu.calculate_z_dev(dz, lds[0], d, lds[1], d, lds[2], n)
        with pytest.raises(zkgpu.ZkgpuError, match="ld < n"):
            zkgpu.calculate_z_block_dev(dz, lds[0], d, lds[1], d, lds[2], n, sc.Z0_LAZY)
        with pytest.raises(zkgpu.ZkgpuError, match="request 1: ld < n"):
            zkgpu.calculate_z_many_dev([(dz, n, d, n, d, n), (dz, lds[0], d, lds[1], d, lds[2])], n)
    assert np.array_equal(fetch(zkgpu, dz), image(3, n)[0])


# ------------------------------------------------------------------ powers of an extension element
@pytest.mark.parametrize("n", sc.EXT_POWERS_N)
def test_ext_powers(oracle, zkgpu, n):
    """1, 2 and 4 workgroups (a thread's step base^T changes with the grid)"""
    ld = n + 5
    for name, base in sc.ext_bases(np.random.default_rng(n)).items():
        exp = sc.oracle_powers3(oracle, base, n)
        if n <= sc.PY_REF_MAX:
            assert np.array_equal(sc.cols3(sc.ref_powers3(base, n)), exp)
        out = dev_out(zkgpu, 3, ld)
        zkgpu.ext_powers_dev(out, ld, np.array(base, dtype=np.uint64), n)
        assert np.array_equal(fetch(zkgpu, out), expect_cols(3, ld, exp)), name
        if name == "zero" and n > 1:
            assert exp[0, 0] == 1 and not exp[:, 1:].any() and not exp[1:, 0].any()


def test_ext_powers_refusal(zkgpu):
    out = dev_out(zkgpu, 3, 8)
    with pytest.raises(zkgpu.ZkgpuError, match="ld < n"):
        zkgpu.ext_powers_dev(out, 7, np.array([2, 3, 4], np.uint64), 8)
    assert np.array_equal(fetch(zkgpu, out), image(3, 8)[0])


# ------------------------------------------------------------------ quotient split
@pytest.mark.parametrize("q_deg", sc.QSPLIT_QDEG)
@pytest.mark.parametrize("n", sc.QSPLIT_N)
def test_qsplit(zkgpu, n, q_deg):
    """lazy inputs and shift; dim 3 / stride 3 through both entry points,
    dim 1 / stride 3 (columns 3p + 1 and 3p + 2 untouched), dim 2 / stride 5;
    dim 0 is a no-op and dim > stride refused"""
    rng = np.random.default_rng([n, q_deg])
    ld1, ld2 = q_deg * n + 3, n + 7
    qq1 = sc.lazy(sc.canonical(rng, (3, q_deg * n)))
    d1 = dev_in(zkgpu, qq1, ld1)
    for shift in (P + 7, int(rng.integers(0, P, dtype=np.uint64))):
        for dim, stride in sc.QSPLIT_DIM_STRIDE:
            ref = sc.ref_qsplit(qq1, n, q_deg, shift, dim, stride)
            at = sorted(ref)
            exp = expect_cols(stride * q_deg, ld2, [np.array(ref[c], dtype=np.uint64) for c in at], at)
            out = dev_out(zkgpu, stride * q_deg, ld2)
            zkgpu.qsplit_cols_dev(out, ld2, d1, ld1, n, q_deg, shift, dim, stride)
            assert np.array_equal(fetch(zkgpu, out), exp), (dim, stride)
            if (dim, stride) == (3, 3):
                out = dev_out(zkgpu, 3 * q_deg, ld2)
                zkgpu.qsplit_dev(out, ld2, d1, ld1, n, q_deg, shift)
                assert np.array_equal(fetch(zkgpu, out), exp)
    out = dev_out(zkgpu, 3 * q_deg, ld2)
    zkgpu.qsplit_cols_dev(out, ld2, d1, ld1, n, q_deg, 7, 0, 3)
    with pytest.raises(zkgpu.ZkgpuError, match="dim 4 > stride 3"):
        zkgpu.qsplit_cols_dev(out, ld2, d1, ld1, n, q_deg, 7, 4, 3)
    assert np.array_equal(fetch(zkgpu, out), image(3 * q_deg, ld2)[0])


def test_qsplit_refusals(zkgpu):
    n, q_deg = 8, 2
    d1 = dev_in(zkgpu, np.ones((3, q_deg * n), np.uint64), q_deg * n)
    out = dev_out(zkgpu, 3 * q_deg, n)
    for ld2, ld1 in ((n - 1, q_deg * n), (n, q_deg * n - 1)):
        with pytest.raises(zkgpu.ZkgpuError, match="ld2 < n or ld1 < q_deg"):
            zkgpu.qsplit_dev(out, ld2, d1, ld1, n, q_deg, 7)
        with pytest.raises(zkgpu.ZkgpuError, match="ld2 < n or ld1 < q_deg"):
            zkgpu.qsplit_cols_dev(out, ld2, d1, ld1, n, q_deg, 7, 1, 3)
    assert np.array_equal(fetch(zkgpu, out), image(3 * q_deg, n)[0])


# ------------------------------------------------------------------ layout changes
@pytest.mark.parametrize("n", sc.COLS3_N)
def test_cols3_to_interleaved(zkgpu, n):
    """words are copied as they are: a lazy word stays lazy"""
    import torch
    ld = n + 9
    cols = sc.lazy(sc.canonical(np.random.default_rng(n), (3, n)))
    out = torch.from_numpy(np.full(3 * n + GUARD, SENT, dtype=np.uint64).view(np.int64)).to("cuda:0")
    zkgpu.cols3_to_interleaved_dev(out, dev_in(zkgpu, cols, ld), ld, n)
    exp = np.full(3 * n + GUARD, SENT, dtype=np.uint64)
    exp[:3 * n] = cols.T.reshape(-1)
    assert np.array_equal(fetch(zkgpu, out), exp)
    assert n < 3 or (exp[:3 * n] >= np.uint64(P)).any()


def test_cols3_to_interleaved_refusal(zkgpu):
    out = dev_out(zkgpu, 3, 8)
    with pytest.raises(zkgpu.ZkgpuError, match="ld < n"):
        zkgpu.cols3_to_interleaved_dev(out, dev_in(zkgpu, np.ones((3, 8), np.uint64), 8), 7, 8)
    assert np.array_equal(fetch(zkgpu, out), image(3, 8)[0])


@pytest.mark.parametrize("nrows,ncols", sc.TRANSPOSE_SHAPES)
def test_transposes(zkgpu, nrows, ncols):
    """32 x 32 tiles ragged in both directions, ld > nrows: both directions
    against the numpy transpose, and the round trip"""
    import torch
    ld = nrows + 3
    rows = np.random.default_rng([nrows, ncols]).integers(0, sc.M64, size=(nrows, ncols), dtype=np.uint64,
                                                           endpoint=True)
    dcols = dev_out(zkgpu, ncols, ld)
    zkgpu.rows_to_cols_dev(dcols, ld, zkgpu.to_device(rows), nrows, ncols)
    assert np.array_equal(fetch(zkgpu, dcols), expect_cols(ncols, ld, rows.T))

    def row_image(r):
        img = np.full(nrows * ncols + GUARD, SENT, dtype=np.uint64)
        img[:nrows * ncols] = r.reshape(-1)
        return img

    # from columns padded with the filler (a read of rows >= nrows would show)
    drows = torch.from_numpy(np.full(nrows * ncols + GUARD, SENT, dtype=np.uint64).view(np.int64)).to("cuda:0")
    zkgpu.cols_to_rows_dev(drows, dev_in(zkgpu, np.ascontiguousarray(rows.T), ld), ld, nrows, ncols)
    assert np.array_equal(fetch(zkgpu, drows), row_image(rows))
    # the round trip through the first call's output
    drows2 = torch.from_numpy(np.full(nrows * ncols + GUARD, SENT, dtype=np.uint64).view(np.int64)).to("cuda:0")
    zkgpu.cols_to_rows_dev(drows2, dcols, ld, nrows, ncols)
    assert np.array_equal(fetch(zkgpu, drows2), row_image(rows))


# ------------------------------------------------------------------ row copies
def _copy(zkgpu, dst_ncols, dst_ld, dst_row0, dst_cols, src, src_row0, src_log_mod, src_cols, ncols, nrows):
    img, view = image(dst_ncols, dst_ld)
    sc.ref_copy_rows(view, dst_row0, dst_cols, src, src_row0, src_log_mod, src_cols, ncols, nrows)
    dst = dev_out(zkgpu, dst_ncols, dst_ld)
    zkgpu.copy_rows_dev(dst, dst_ld, dst_row0, dst_cols, zkgpu.to_device(src), src.shape[1], src_row0, src_log_mod,
                        src_cols, ncols, nrows)
    assert np.array_equal(fetch(zkgpu, dst), img)
    return img


@pytest.mark.parametrize("nrows", sc.COPY_NROWS)
def test_copy_rows(zkgpu, nrows):
    rng = np.random.default_rng(nrows)
    dst_row0, src_row0 = 3, 2
    dst_ld = dst_row0 + nrows + 5
    src = rng.integers(0, sc.M64, size=(3, src_row0 + nrows + 4), dtype=np.uint64, endpoint=True)
    # identity column lists, no wrap
    a = _copy(zkgpu, 4, dst_ld, dst_row0, None, src, src_row0, 0, None, 3, nrows)
    assert np.array_equal(a[:4 * dst_ld].reshape(4, dst_ld)[:3, dst_row0:dst_row0 + nrows],
                          src[:, src_row0:src_row0 + nrows])
    # given lists: not monotonic, one source column named twice; columns 1 and 4 untouched
    _copy(zkgpu, 5, dst_ld, dst_row0, [3, 0, 2], src, src_row0, 0, [1, 1, 0], 3, nrows)
    # a window that crosses 2^src_log_mod and wraps
    log_mod, wrap_row0, src_ld = sc.copy_wrap(nrows)
    wsrc = rng.integers(0, sc.M64, size=(3, src_ld), dtype=np.uint64, endpoint=True)
    b = _copy(zkgpu, 5, dst_ld, dst_row0, [4, 1, 2], wsrc, wrap_row0, log_mod, [2, 0, 2], 3, nrows)
    last = b[:5 * dst_ld].reshape(5, dst_ld)[1, dst_row0 + nrows - 1]
    assert last == wsrc[0, (wrap_row0 + nrows - 1) - (1 << log_mod)]
    # no-ops
    _copy(zkgpu, 4, dst_ld, dst_row0, None, src, src_row0, 0, None, 0, nrows)
    _copy(zkgpu, 4, dst_ld, dst_row0, [3, 0, 2], src, src_row0, 0, [1, 1, 0], 3, 0)


def test_copy_rows_refusals(zkgpu):
    src = np.ones((3, 16), np.uint64)
    dsrc = zkgpu.to_device(src)
    dst = dev_out(zkgpu, 3, 16)
    for dst_row0, src_row0, src_ld, log_mod in ((9, 0, 16, 0),    # rows beyond dst_ld
                                                (0, 9, 16, 0),    # rows beyond src_ld
                                                (0, 0, 15, 4)):   # 2^src_log_mod > src_ld
        with pytest.raises(zkgpu.ZkgpuError, match="outside the buffers' leading dimensions"):
            zkgpu.copy_rows_dev(dst, 16, dst_row0, None, dsrc, src_ld, src_row0, log_mod, None, 3, 8)
    assert np.array_equal(fetch(zkgpu, dst), image(3, 16)[0])


# ------------------------------------------------------------------ PRNG columns
@pytest.mark.parametrize("nrows", sc.RAND_NROWS)
def test_rand_cols(zkgpu, nrows):
    """a column list with gaps, out of order: unlisted columns keep the
    sentinel; the row-block form with row0 + nrows crossing 2^log_n (the halo
    rows wrap to the domain's first rows)"""
    cols, ncols, ld, seed = [5, 0, 3], 7, nrows + 2, 0x1234567 + nrows
    img, view = image(ncols, ld)
    sc.ref_rand_cols(view, cols, 0, nrows, None, seed, 1)
    out = dev_out(zkgpu, ncols, ld)
    zkgpu.rand_cols_dev(out, ld, cols, nrows, seed, 1)
    assert np.array_equal(fetch(zkgpu, out), img)
    row0 = sc.rand_block_row0(nrows)
    img, view = image(ncols, ld)
    sc.ref_rand_cols(view, cols, row0, nrows, sc.RAND_LOG_N, seed, 0)
    out = dev_out(zkgpu, ncols, ld)
    zkgpu.rand_cols_rows_dev(out, ld, cols, row0, nrows, sc.RAND_LOG_N, seed, 0)
    assert np.array_equal(fetch(zkgpu, out), img)
    # the wrapped rows are the domain's first rows
    first, _ = image(ncols, ld)
    sc.ref_rand_cols(first[:ncols * ld].reshape(ncols, ld), cols, 0, 1, None, seed, 0)
    k = (1 << sc.RAND_LOG_N) - row0
    assert view[5, k] == first[5 * ld]


def test_rand_cols_refusals(zkgpu):
    out = dev_out(zkgpu, 3, 8)
    with pytest.raises(zkgpu.ZkgpuError, match="rand_cols_rows: bad shape"):
        zkgpu.rand_cols_rows_dev(out, 8, [0, 2], 0, 9, 4, 1, 0)
    with pytest.raises(zkgpu.ZkgpuError, match="rand_cols: bad shape"):
        zkgpu.rand_cols_dev(out, 8, [0, 2], 9, 1, 0)
    with pytest.raises(zkgpu.ZkgpuError, match="rand_cols: bad shape"):
        zkgpu.rand_cols_dev(out, 8, np.zeros(65536, np.uint32), 8, 1, 0)
    assert np.array_equal(fetch(zkgpu, out), image(3, 8)[0])
