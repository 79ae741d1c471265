"""The evaluation, FRI and opening primitives on the GPU at ragged shapes.

Stage 5 and the FRI / query phase through their C-ABI entry points, at the
sizes of tests/xi_cases.py (checked on the CPU by tests/test_xi_cases.py).
Every comparison is bit-exact against the reference on the inputs reduced mod
p.  Every output buffer starts as a sentinel word and carries a guard; whole
buffers are compared, so a stray write shows.  Input columns carry a filler
in the rows and columns a call must not read, which an over-read or a wrong
stride would fold into the result.  Every xi and special_x has non-zero
second and third components, so no denominator vanishes.

What each size list straddles:

- zkgpu_lagrange_xi_rows_dev, zkgpu_xdivxsub_dev, zkgpu_xdivxsub_rows_dev
  (k_xdiv_rows): BI_CHUNK = 16 rows of a thread share one inversion (15, 16,
  17 rows; one row); 256 threads x 16 = 4096 rows fill one workgroup, 4097
  double the stride T between a thread's rows; a block that ends exactly at
  N, the whole domain, an empty block; row0 enters the twiddle exponent
  ((row0 + k) mod N) << (28 - n_bits): n_bits 0 and 1 (one twiddle), 24 and 28
  (a non-zero index into the low table times the high table, up to its last
  entry); the prover's form, lev + row0 in an ld = N buffer.
- zkgpu_evmap_dev (k_evmap_groups, k_evmap_sum_subs): 256 threads; 512 rows
  per iteration at UR = 2; 61440 = evmap_rows_per_block() (one block, exactly
  one, a second block of one row that k_evmap_sum_subs must add); the host's
  grouping by prime into groups of GW = 4 sub-entries (exactly one group, a
  group and one, a dim-3 entry across two groups, one prime only, one column
  under both primes, 45 entries, none); extend_bits 0 and 2 with a leading
  dimension per entry; the prover's row blocks with the pointers advanced.
- zkgpu_fri_fold_dev / zkgpu_fri_fold_rows_dev (k_fri_fold): every reduction
  0..5 (a template instance each) at out_bits 0 and 1 (fewer groups than a
  wave), two workgroups; pol_bits 16, 24, 28 with the twiddle exponent
  g << (28 - pol_bits) crossing a multiple of 2^14 inside the block (low
  table wraps, high index steps), the last groups of the fold, 257 groups
  (one thread in the second workgroup).
- zkgpu_fri_transpose_dev: width 1, height 1, wide, tall, a ragged last
  workgroup.
- zkgpu_gl_merkle_open_dev / _open_rows_dev / _open_many (k_merkle_open): 64
  threads loop over the columns (0, 63, 64, 65, 130 columns); 1 row (no
  level, empty siblings), 2, 4, 1024 rows; ld > nrows; repeated, unsorted
  indices; 1 and 300 queries.
"""
import ctypes
import functools

import numpy as np
import pytest

import stage_cases as sc
import xi_cases as xc
from test_gpu_stage_primitives import FILL, GUARD, SENT, dev_in, dev_out, expect_cols, fetch, image

pytestmark = pytest.mark.gpu

P = xc.P


def addr(t, words=0):
    """device address `words` words into a tensor"""
    return t.data_ptr() + 8 * words


def flat_image(nwords, at=0, words=None):
    """an untouched nwords-word output (plus guard) with `words` at offset `at`"""
    img, _ = image(1, nwords)
    if words is not None:
        w = np.asarray(words, dtype=np.uint64).reshape(-1)
        img[at:at + w.size] = w
    return img


def u64s(rows):
    return np.array(rows, dtype=np.uint64).reshape(-1, 3)


# ------------------------------------------------------------------ LEv / LpEv
XI = xc.rand_xi(np.random.default_rng(13))


@functools.lru_cache(maxsize=None)
def lag_whole(n_bits, xi):
    """(LEv, LpEv) of the whole domain as (3, N) columns; computed once"""
    lev, lpev = xc.ref_lagrange(xi, n_bits, range(1 << n_bits))
    out = sc.cols3(lev), sc.cols3(lpev)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("row0,nrows", xc.LAG_BLOCKS)
def test_lagrange_xi_rows_blocks(zkgpu, row0, nrows):
    """each block into its own buffer (ld = nrows + 5), and the way the prover
    calls it: at base + row0 of a 3-column, ld = N buffer whose other rows keep
    the sentinel"""
    n_bits, n = xc.LAG_NBITS, 1 << xc.LAG_NBITS
    ref = [w[:, row0:row0 + nrows] for w in lag_whole(n_bits, XI)]
    ld = nrows + 5
    lev, lpev = dev_out(zkgpu, 3, ld), dev_out(zkgpu, 3, ld)
    zkgpu.lagrange_xi_rows_dev(lev, lpev, ld, np.array(XI, np.uint64), n_bits, row0, nrows)
    assert np.array_equal(fetch(zkgpu, lev), expect_cols(3, ld, ref[0]))
    assert np.array_equal(fetch(zkgpu, lpev), expect_cols(3, ld, ref[1]))
    lev, lpev = dev_out(zkgpu, 3, n), dev_out(zkgpu, 3, n)
    zkgpu.lagrange_xi_rows_dev(addr(lev, row0), addr(lpev, row0), n, np.array(XI, np.uint64), n_bits, row0, nrows)
    for got, r in ((lev, ref[0]), (lpev, ref[1])):
        img, v = image(3, n)
        v[:, row0:row0 + nrows] = r
        assert np.array_equal(fetch(zkgpu, got), img)


@pytest.mark.parametrize("n_bits", xc.LAG_SMALL_NBITS)
def test_lagrange_xi_rows_small_domains_lazy_xi(zkgpu, n_bits):
    """the whole domain at 1, 2 and 16 rows; a lazy xi gives the result of the reduced xi"""
    n = 1 << n_bits
    ld = n + 5
    ref = lag_whole(n_bits, sc.f3(xc.XI_LAZY))
    for xi in (xc.XI_LAZY, sc.f3(xc.XI_LAZY)):
        lev, lpev = dev_out(zkgpu, 3, ld), dev_out(zkgpu, 3, ld)
        zkgpu.lagrange_xi_rows_dev(lev, lpev, ld, np.array(xi, np.uint64), n_bits, 0, n)
        assert np.array_equal(fetch(zkgpu, lev), expect_cols(3, ld, ref[0])), xi
        assert np.array_equal(fetch(zkgpu, lpev), expect_cols(3, ld, ref[1])), xi
    if n_bits == 0:
        assert ref[0][:, 0].tolist() == [1, 0, 0]


@pytest.mark.parametrize("n_bits", xc.LAG_BIG_NBITS)
def test_lagrange_xi_rows_large_domains(zkgpu, n_bits):
    """2^24 and 2^28 rows: blocks at the start, the end and the middle of the
    domain against the closed form (nothing of the domain's size is allocated)"""
    for row0, nrows in xc.big_blocks(n_bits):
        ref = xc.ref_lagrange(XI, n_bits, range(row0, row0 + nrows))
        ld = nrows + 5
        lev, lpev = dev_out(zkgpu, 3, ld), dev_out(zkgpu, 3, ld)
        zkgpu.lagrange_xi_rows_dev(lev, lpev, ld, np.array(XI, np.uint64), n_bits, row0, nrows)
        assert np.array_equal(fetch(zkgpu, lev), expect_cols(3, ld, sc.cols3(ref[0]))), (row0, nrows)
        assert np.array_equal(fetch(zkgpu, lpev), expect_cols(3, ld, sc.cols3(ref[1]))), (row0, nrows)


def test_lagrange_xi_rows_refusals(zkgpu):
    n_bits, n = 4, 16
    lev, lpev = dev_out(zkgpu, 3, n), dev_out(zkgpu, 3, n)
    xi = np.array(XI, np.uint64)
    for row0, nrows, ld in ((n + 1, 0, n),      # row0 > N
                            (9, 8, n),          # nrows > N - row0
                            (0, 8, 7)):         # ld < nrows
        with pytest.raises(zkgpu.ZkgpuError, match="outside the domain or ld too small"):
            zkgpu.lagrange_xi_rows_dev(lev, lpev, ld, xi, n_bits, row0, nrows)
    with pytest.raises(zkgpu.ZkgpuError, match="lagrange_xi_rows: bits"):
        zkgpu.lagrange_xi_rows_dev(lev, lpev, n, xi, 29, 0, 1)
    assert sc.f3(xc.XI_BASE_LAZY) == (5, 0, 0)
    with pytest.raises(zkgpu.ZkgpuError, match="base field"):
        zkgpu.lagrange_xi_rows_dev(lev, lpev, n, np.array(xc.XI_BASE_LAZY, np.uint64), n_bits, 0, n)
    assert np.array_equal(fetch(zkgpu, lev), image(3, n)[0])
    assert np.array_equal(fetch(zkgpu, lpev), image(3, n)[0])


# ------------------------------------------------------------------ xDivXSub
@functools.lru_cache(maxsize=None)
def xdiv_whole(n_bits, n_bits_ext, xi):
    """(xdiv, xdivw) of the whole extended domain, interleaved (NE x 3); computed once"""
    a, b = xc.ref_xdivxsub(xi, n_bits, n_bits_ext, range(1 << n_bits_ext))
    out = u64s(a), u64s(b)
    for r in out:
        r.setflags(write=False)
    return out


@pytest.mark.parametrize("n_bits,n_bits_ext", xc.XDIV_ROWS_BITS)
def test_xdivxsub_rows(zkgpu, n_bits, n_bits_ext):
    """the row blocks of xi_cases.row_blocks, scaled to the domain: both
    outputs over the whole 3 NE + guard buffer; nrows = 0 changes nothing"""
    ne = 1 << n_bits_ext
    ref = xdiv_whole(n_bits, n_bits_ext, sc.f3(xc.XI_LAZY))
    for row0, nrows in xc.row_blocks(ne):
        da, db = dev_out(zkgpu, 1, 3 * ne), dev_out(zkgpu, 1, 3 * ne)
        zkgpu.xdivxsub_rows_dev(da, db, np.array(sc.f3(xc.XI_LAZY), np.uint64), n_bits, n_bits_ext, row0, nrows)
        for got, r in ((da, ref[0]), (db, ref[1])):
            assert np.array_equal(fetch(zkgpu, got), flat_image(3 * ne, 3 * row0, r[row0:row0 + nrows])), (row0, nrows)


@pytest.mark.parametrize("n_bits,n_bits_ext", xc.XDIV_WHOLE_BITS)
def test_xdivxsub_whole_lazy_xi(zkgpu, n_bits, n_bits_ext):
    ne = 1 << n_bits_ext
    ref = xdiv_whole(n_bits, n_bits_ext, sc.f3(xc.XI_LAZY))
    da, db = dev_out(zkgpu, 1, 3 * ne), dev_out(zkgpu, 1, 3 * ne)
    zkgpu.xdivxsub_dev(da, db, np.array(xc.XI_LAZY, np.uint64), n_bits, n_bits_ext)
    assert np.array_equal(fetch(zkgpu, da), flat_image(3 * ne, 0, ref[0]))
    assert np.array_equal(fetch(zkgpu, db), flat_image(3 * ne, 0, ref[1]))


def test_xdivxsub_refusals(zkgpu):
    nb, nbe, ne = 3, 4, 16
    da, db = dev_out(zkgpu, 1, 3 * ne), dev_out(zkgpu, 1, 3 * ne)
    xi = np.array(XI, np.uint64)
    for row0, nrows in ((ne + 1, 0), (ne - 1, 2), (0, ne + 1)):
        with pytest.raises(zkgpu.ZkgpuError, match="outside the domain"):
            zkgpu.xdivxsub_rows_dev(da, db, xi, nb, nbe, row0, nrows)
    for bits in ((nbe + 1, nbe), (3, 29)):
        with pytest.raises(zkgpu.ZkgpuError, match="xdivxsub_rows: bits"):
            zkgpu.xdivxsub_rows_dev(da, db, xi, bits[0], bits[1], 0, 1)
        with pytest.raises(zkgpu.ZkgpuError, match="xdivxsub: bits"):
            zkgpu.xdivxsub_dev(da, db, xi, bits[0], bits[1])
    assert np.array_equal(fetch(zkgpu, da), image(1, 3 * ne)[0])
    assert np.array_equal(fetch(zkgpu, db), image(1, 3 * ne)[0])


# ------------------------------------------------------------------ evmap
@functools.lru_cache(maxsize=None)
def ev_case(n, eb, name):
    return xc.EvCase(n, eb, xc.EV_LISTS[name])


def ev_expected(oracle, case, r0=0, r1=None):
    """Python integers up to PY_REF_MAX rows (and the oracle agrees), the oracle beyond"""
    ref = xc.oracle_evmap(oracle, case, r0, r1)
    if (case.n if r1 is None else r1) - r0 <= xc.PY_REF_MAX:
        assert np.array_equal(xc.ref_evmap(case, r0, r1), ref)
    return ref


class EvDevice:
    """the case on the device: lev / lpev at ld = n + 7 with the filler in the
    rows >= n; every polynomial at its own ld, the filler in the rows past
    (n - 1) << eb and in every row that is no multiple of 2^eb"""

    def __init__(self, zkgpu, case):
        self.case = case
        self.l_ld = xc.ev_l_ld(case.n)
        self.lev = dev_in(zkgpu, case.lev, self.l_ld)
        self.lpev = dev_in(zkgpu, case.lpev, self.l_ld)
        self.polys = {poly: zkgpu.to_device(case.poly_image(poly, FILL, GUARD)) for poly in case.polys}
        self.lds = [case.ld[poly] for poly, _, _ in case.entries]

    def call(self, zkgpu, r0=0, r1=None, l_ld=None, lds=None):
        """rows [r0, r1): the pointers advanced, the leading dimensions kept"""
        case = self.case
        r1 = case.n if r1 is None else r1
        cols = [addr(self.polys[poly], r0 << case.eb) for poly, _, _ in case.entries]
        return zkgpu.evmap_dev(cols, self.lds if lds is None else lds, case.dims, case.primes, addr(self.lev, r0),
                               addr(self.lpev, r0), self.l_ld if l_ld is None else l_ld, r1 - r0, case.eb)


@pytest.mark.parametrize("eb", xc.EV_EB)
@pytest.mark.parametrize("n", xc.EV_N)
def test_evmap_shapes(oracle, zkgpu, n, eb):
    case = ev_case(n, eb, "shape")
    got = EvDevice(zkgpu, case).call(zkgpu)
    want = ev_expected(oracle, case)
    print("n=%d eb=%d\n%s\n%s" % (n, eb, got, want))
    assert got.dtype == want.dtype and np.array_equal(got, want)


@pytest.mark.parametrize("eb", xc.EV_EB)
@pytest.mark.parametrize("name", sorted(xc.EV_LISTS))
def test_evmap_entry_lists(oracle, zkgpu, name, eb):
    case = ev_case(xc.EV_LIST_N, eb, name)
    got = EvDevice(zkgpu, case).call(zkgpu)
    want = ev_expected(oracle, case)
    assert got.shape == (len(xc.EV_LISTS[name]), 3) and np.array_equal(got, want)


@pytest.mark.parametrize("eb", xc.EV_EB)
def test_evmap_row_blocks_as_the_prover_calls_them(oracle, zkgpu, eb):
    """[0, k) and [k, n) with lev + k, col + (k << eb) and the whole columns'
    leading dimensions: each equals its reference and they add up to the whole call"""
    n, k = xc.EV_SPLIT
    case = ev_case(n, eb, "shape")
    dev = EvDevice(zkgpu, case)
    whole, lo, hi = dev.call(zkgpu), dev.call(zkgpu, 0, k), dev.call(zkgpu, k, n)
    assert np.array_equal(lo, ev_expected(oracle, case, 0, k))
    assert np.array_equal(hi, ev_expected(oracle, case, k, n))
    assert np.array_equal(whole, ev_expected(oracle, case))
    assert np.array_equal(xc.add_evals(lo, hi), whole)


def test_evmap_refusals_and_empty_block(zkgpu):
    n, eb = 64, 2
    case = ev_case(n, eb, "dim3_straddles")
    dev = EvDevice(zkgpu, case)
    with pytest.raises(zkgpu.ZkgpuError, match="l_ld < n"):
        dev.call(zkgpu, l_ld=n - 1)
    # the dim-3 entry (index 2): one row short of ((n - 1) << eb) + 1
    short = list(dev.lds)
    short[2] = xc.ev_span(n, eb) - 1
    with pytest.raises(zkgpu.ZkgpuError, match="entry 2: ld"):
        dev.call(zkgpu, lds=short)
    # exactly the rows read is enough, and a dim-1 entry's ld is not used
    tight = xc.EvCase(n, eb, xc.EV_LISTS["dim3_straddles"])
    tight.ld = {poly: xc.ev_span(n, eb) for poly in tight.ld}
    tdev = EvDevice(zkgpu, tight)
    lds = list(tdev.lds)
    lds[0] = 0
    assert np.array_equal(tdev.call(zkgpu, lds=lds), xc.ref_evmap(tight))
    # n = 0: zero evaluations, nothing launched; the ld checks do not apply to an empty block
    got = dev.call(zkgpu, 5, 5, l_ld=0)
    assert got.shape == (4, 3) and not got.any()


# ------------------------------------------------------------------ FRI fold
def fold_args(rng):
    """(special_x lazy, its reduced form, shift_inv >= p, its reduced form)"""
    sx = xc.lazy_ext(rng)
    sinv = xc.fold_shift_inv(rng)
    return np.array(sx, np.uint64), np.array(sc.f3(sx), np.uint64), sinv, sinv % P


@pytest.mark.parametrize("pol_bits,out_bits", xc.FOLD_WHOLE)
def test_fri_fold_lazy_small_outputs(oracle, zkgpu, pol_bits, out_bits):
    rng = np.random.default_rng([pol_bits, out_bits])
    canon = xc.canonical(rng, 3 << pol_bits)
    sx, sx_c, sinv, sinv_c = fold_args(rng)
    want = oracle.fri_fold(canon, pol_bits, out_bits, sx_c, sinv_c)
    out = dev_out(zkgpu, 1, 3 << out_bits)
    zkgpu.fri_fold_dev(out, zkgpu.to_device(xc.lazy(canon)), pol_bits, out_bits, sx, sinv)
    assert np.array_equal(fetch(zkgpu, out), flat_image(3 << out_bits, 0, want))


@pytest.mark.parametrize("reduction", xc.FOLD_ROWS_REDUCTION)
@pytest.mark.parametrize("pol_bits", xc.FOLD_ROWS_BITS)
def test_fri_fold_rows_large_domains(oracle, zkgpu, pol_bits, reduction):
    """groups [g0, g0 + ng) of a 2^pol_bits fold from their rows alone: the
    first groups, the last, and a block across a step of the high twiddle index"""
    out_bits = pol_bits - reduction
    nx = 1 << reduction
    for ng in xc.FOLD_ROWS_NG:
        for g0 in xc.fold_rows_g0(pol_bits, out_bits, ng):
            rng = np.random.default_rng([pol_bits, reduction, ng, g0])
            canon = xc.canonical(rng, (ng, 3 * nx))
            sx, sx_c, sinv, sinv_c = fold_args(rng)
            want = np.stack([oracle.fri_fold_group(canon[j], g0 + j, pol_bits, sx_c, sinv_c) for j in range(ng)])
            out = dev_out(zkgpu, 1, 3 * ng)
            zkgpu.fri_fold_rows_dev(out, zkgpu.to_device(xc.lazy(canon)), g0, ng, pol_bits, out_bits, sx, sinv)
            assert np.array_equal(fetch(zkgpu, out), flat_image(3 * ng, 0, want)), (ng, g0)


def test_fri_fold_refusals(zkgpu):
    rng = np.random.default_rng(5)
    pol = zkgpu.to_device(xc.canonical(rng, 3 << 8))
    out = dev_out(zkgpu, 1, 3 << 8)
    sx, _, sinv, _ = fold_args(rng)
    with pytest.raises(zkgpu.ZkgpuError, match="bad bits 4 -> 5"):
        zkgpu.fri_fold_dev(out, pol, 4, 5, sx, sinv)
    with pytest.raises(zkgpu.ZkgpuError, match="bad bits 29 -> 27"):
        zkgpu.fri_fold_rows_dev(out, pol, 0, 1, 29, 27, sx, sinv)
    with pytest.raises(zkgpu.ZkgpuError, match="reduction of 6 bits > 5 unsupported"):
        zkgpu.fri_fold_dev(out, pol, 8, 2, sx, sinv)
    with pytest.raises(zkgpu.ZkgpuError, match="reduction of 6 bits > 5 unsupported"):
        zkgpu.fri_fold_rows_dev(out, pol, 0, 1, 8, 2, sx, sinv)
    with pytest.raises(zkgpu.ZkgpuError, match=r"groups \[60, \+5\) outside the 2\^6 outputs"):
        zkgpu.fri_fold_rows_dev(out, pol, 60, 5, 8, 6, sx, sinv)
    with pytest.raises(zkgpu.ZkgpuError, match=r"groups \[18446744073709551615, \+2\) outside the 2\^6 outputs"):
        zkgpu.fri_fold_rows_dev(out, pol, xc.M64, 2, 8, 6, sx, sinv)
    zkgpu.fri_fold_rows_dev(out, pol, 64, 0, 8, 6, sx, sinv)  # ng = 0 at the end of the outputs: nothing to do
    zkgpu.fri_fold_rows_dev(out, pol, 7, 0, 8, 6, sx, sinv)
    assert np.array_equal(fetch(zkgpu, out), image(1, 3 << 8)[0])


# ------------------------------------------------------------------ FRI transpose
@pytest.mark.parametrize("degree,tbits", xc.FRI_TRANSPOSE)
def test_fri_transpose_shapes(oracle, zkgpu, degree, tbits):
    """words move as they are: the numpy transpose of the raw (lazy) words;
    on canonical words the oracle's getTransposed"""
    w, h = 1 << tbits, degree >> tbits
    canon = xc.canonical(np.random.default_rng([degree, tbits]), 3 * degree)
    for pol in (xc.lazy(canon), canon):
        aux = dev_out(zkgpu, 1, 3 * degree)
        zkgpu.fri_transpose_dev(aux, zkgpu.to_device(pol), degree, tbits)
        got = fetch(zkgpu, aux)
        assert np.array_equal(got, flat_image(3 * degree, 0, pol.reshape(h, w, 3).transpose(1, 0, 2)))
    assert np.array_equal(got[:3 * degree], oracle.fri_get_transposed(canon, tbits))


def test_fri_transpose_refusal_and_empty(zkgpu):
    pol = zkgpu.to_device(xc.canonical(np.random.default_rng(6), 3 * 12))
    aux = dev_out(zkgpu, 1, 3 * 12)
    with pytest.raises(zkgpu.ZkgpuError, match="degree not a multiple of 2\\^3"):
        zkgpu.fri_transpose_dev(aux, pol, 12, 3)
    zkgpu.fri_transpose_dev(aux, pol, 0, 0)
    zkgpu.fri_transpose_dev(aux, pol, 0, 3)
    assert np.array_equal(fetch(zkgpu, aux), image(1, 3 * 12)[0])


# ------------------------------------------------------------------ openings
def open_outputs(nq, ncols, nlev):
    """host outputs of one request: sentinel words and a guard behind each"""
    return (np.full(nq * ncols + GUARD, SENT, dtype=np.uint64), np.full(nq * nlev * 4 + GUARD, SENT, dtype=np.uint64))


def open_call(zkgpu, kind, nodes, src, ld, ncols, nrows, idx):
    """merkle_open_dev ("cols") / merkle_open_rows_dev ("rows") / one request
    of merkle_open_many ("many_cols", "many_rows") into sentinel-filled host
    buffers -> (vals image, sibs image)"""
    idx = np.ascontiguousarray(idx, dtype=np.uint64)
    nlev = max(0, int(nrows).bit_length() - 1)
    vals, sibs = open_outputs(idx.size, ncols, nlev)
    L = zkgpu.lib()
    if kind == "cols":
        rc = L.zkgpu_gl_merkle_open_dev(vals.ctypes.data, sibs.ctypes.data, addr(nodes), addr(src), ld, ncols, nrows,
                                        idx.ctypes.data, idx.size)
    elif kind == "rows":
        rc = L.zkgpu_gl_merkle_open_rows_dev(vals.ctypes.data, sibs.ctypes.data, addr(nodes), addr(src), ncols, nrows,
                                             idx.ctypes.data, idx.size)
    else:
        req = (zkgpu.OpenReq * 1)(zkgpu.OpenReq(vals.ctypes.data, sibs.ctypes.data, addr(nodes), addr(src), ld, ncols,
                                                nrows, idx.ctypes.data, idx.size, 1 if kind == "many_rows" else 0))
        rc = L.zkgpu_gl_merkle_open_many(req, 1)
    if rc:
        raise zkgpu.ZkgpuError(L.zkgpu_last_error().decode(errors="replace"))
    return vals, sibs


def open_expected(oracle, ref_nodes, src, idx):
    nrows, ncols = src.shape
    nlev = max(0, nrows.bit_length() - 1)
    vals, sibs = open_outputs(len(idx), ncols, nlev)
    for q, i in enumerate(idx):
        v, s = oracle.merkle_group_proof(ref_nodes, src, int(i))
        assert s.shape == (nlev, 4)
        vals[q * ncols:(q + 1) * ncols] = v
        sibs[q * nlev * 4:(q + 1) * nlev * 4] = s.reshape(-1)
    return vals, sibs


@pytest.mark.parametrize("ncols", xc.OPEN_NCOLS)
@pytest.mark.parametrize("nrows", xc.OPEN_NROWS)
def test_merkle_openings(oracle, zkgpu, nrows, ncols):
    """the oracle's tree, uploaded: the opening kernel by itself.  A
    column-major source at ld = nrows + 3 (filler below the rows) and a
    row-major one, each through its own entry point and through open_many,
    and both in one open_many call"""
    rng = np.random.default_rng([nrows, ncols])
    src = xc.canonical(rng, (nrows, ncols))
    ref_nodes = oracle.merkletree(src)
    nodes = zkgpu.to_device(ref_nodes)
    ld = nrows + 3
    # (no columns: any valid address, nothing is read from it)
    dcols = dev_in(zkgpu, np.ascontiguousarray(src.T), ld) if ncols else nodes
    drows = zkgpu.to_device(np.concatenate([src.reshape(-1), np.full(GUARD, FILL, np.uint64)])) if ncols else nodes
    for nq in xc.OPEN_NQ:
        idx = xc.open_indices(nrows, nq, rng)
        want = open_expected(oracle, ref_nodes, src, idx)
        if nrows == 1:
            assert want[1].size == GUARD and np.array_equal(want[0][:nq * ncols], np.tile(src[0], nq))
        for kind, dsrc in (("cols", dcols), ("rows", drows), ("many_cols", dcols), ("many_rows", drows)):
            vals, sibs = open_call(zkgpu, kind, nodes, dsrc, ld, ncols, nrows, idx)
            assert np.array_equal(vals, want[0]), (kind, nq)
            assert np.array_equal(sibs, want[1]), (kind, nq)
        # both kinds in one call, through the binding
        (v0, s0), (v1, s1) = zkgpu.merkle_open_many([(nodes, dcols, ld, ncols, nrows, idx, False),
                                                     (nodes, drows, 0, ncols, nrows, idx[::-1], True)])
        nlev = s0.shape[1]
        assert np.array_equal(v0.reshape(-1), want[0][:nq * ncols]) and np.array_equal(v1, v0[::-1])
        assert np.array_equal(s0.reshape(-1), want[1][:nq * nlev * 4]) and np.array_equal(s1, s0[::-1])


def test_merkle_open_refusals(oracle, zkgpu):
    """nrows that is no power of two, and an index out of range anywhere in
    the list: refused before anything is queued, the outputs untouched"""
    rng = np.random.default_rng(9)
    src = xc.canonical(rng, (8, 5))
    nodes = zkgpu.to_device(oracle.merkletree(src))
    dcols = dev_in(zkgpu, np.ascontiguousarray(src.T), 8)
    drows = zkgpu.to_device(src)
    for kind, dsrc in (("cols", dcols), ("rows", drows), ("many_cols", dcols), ("many_rows", drows)):
        for nrows in (6, 0, 7):
            with pytest.raises(zkgpu.ZkgpuError, match="nrows %d is not a power of two" % nrows):
                open_call(zkgpu, kind, nodes, dsrc, 8, 5, nrows, np.array([0, 1], np.uint64))
        with pytest.raises(zkgpu.ZkgpuError, match="index 8 >= nrows"):
            open_call(zkgpu, kind, nodes, dsrc, 8, 5, 8, np.array([0, 7, 8, 1], np.uint64))
    # the outputs of a refused call keep their words
    idx = np.array([3, 9], np.uint64)
    vals, sibs = open_outputs(2, 5, 3)
    L = zkgpu.lib()
    assert L.zkgpu_gl_merkle_open_dev(vals.ctypes.data, sibs.ctypes.data, addr(nodes), addr(dcols), 8, 5, 8,
                                      idx.ctypes.data, 2) != 0
    assert L.zkgpu_gl_merkle_open_rows_dev(vals.ctypes.data, sibs.ctypes.data, addr(nodes), addr(drows), 5, 8,
                                           idx.ctypes.data, 2) != 0
    assert (vals == SENT).all() and (sibs == SENT).all()
