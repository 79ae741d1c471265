"""CPU checks of tests/xi_cases.py: the closed forms of LEv / LpEv and xDivXSub
and the Python-integer evmap equal the oracle wherever the oracle reaches, the
oracle's per-group fold equals its whole fold, and every size list really
straddles the launch constant it names."""
import numpy as np
import pytest

import stage_cases as sc
import xi_cases as xc

P = xc.P


# ------------------------------------------------------------------ references vs the oracle
def test_gl_w_matches_oracle(oracle):
    for n_bits in range(0, 33):
        assert xc.gl_w(n_bits) == oracle.gl_w(n_bits), n_bits
    assert xc.f3_pow((2, 3, 5), 0) == sc.ONE3
    assert xc.f3_pow((2, 3, 5), 5) == sc.ref_powers3((2, 3, 5), 6)[5]


def test_xi_constants():
    assert sc.f3(xc.XI_LAZY) == (3, 2**32 - 2, 1) and min(xc.XI_LAZY) >= P
    assert sc.f3(xc.XI_BASE_LAZY) == (5, 0, 0) and xc.XI_BASE_LAZY[1] != 0
    rng = np.random.default_rng(0)
    for _ in range(20):
        for x in (xc.rand_xi(rng), xc.lazy_ext(rng)):
            assert x[1] % P and x[2] % P and max(x) <= xc.M64
        assert min(xc.lazy_ext(rng)) >= P
        assert P <= xc.fold_shift_inv(rng) <= xc.M64


@pytest.mark.parametrize("n_bits", range(0, 12))
def test_ref_lagrange_matches_intt_of_powers(oracle, n_bits):
    """starks.cpp:308-324: LEv = INTT_N of the powers of xi, LpEv of those of w_N xi"""
    n = 1 << n_bits
    for xi in (xc.rand_xi(np.random.default_rng(n_bits)), xc.XI_LAZY):
        lev, lpev = xc.ref_lagrange(xi, n_bits, range(n))
        wxi = xc.f3_scale(sc.f3(xi), xc.gl_w(n_bits))
        for got, base in ((lev, sc.f3(xi)), (lpev, wxi)):
            pw = np.ascontiguousarray(sc.oracle_powers3(oracle, base, n).T)
            assert np.array_equal(np.array(got, dtype=np.uint64).reshape(n, 3), oracle.ntt(pw, inverse=True))


@pytest.mark.parametrize("n_bits_ext", range(0, 12))
def test_ref_xdivxsub_matches_oracle(oracle, n_bits_ext):
    ne = 1 << n_bits_ext
    xi = xc.rand_xi(np.random.default_rng(100 + n_bits_ext))
    x = np.zeros(ne, np.uint64)
    oracle.lib().oc_powers(oracle._p(x), 7, oracle.gl_w(n_bits_ext), ne)
    xia = np.array(xi, dtype=np.uint64)
    for n_bits in range(0, n_bits_ext + 1):
        a = np.zeros((ne, 3), np.uint64)
        b = np.zeros((ne, 3), np.uint64)
        oracle.lib().oc_xdivxsub(oracle._p(a), oracle._p(b), oracle._p(x), ne, oracle._p(xia), oracle.gl_w(n_bits))
        ra, rb = xc.ref_xdivxsub(xi, n_bits, n_bits_ext, range(ne))
        assert np.array_equal(np.array(ra, dtype=np.uint64).reshape(ne, 3), a), n_bits
        assert np.array_equal(np.array(rb, dtype=np.uint64).reshape(ne, 3), b), n_bits


def test_ref_rows_are_the_whole_domains_rows():
    """a row list gives those rows of the whole domain (the form the large domains use)"""
    xi = xc.rand_xi(np.random.default_rng(7))
    whole = xc.ref_lagrange(xi, 9, range(512))
    part = xc.ref_lagrange(xi, 9, range(500, 512))
    assert part[0] == whole[0][500:] and part[1] == whole[1][500:]
    whole = xc.ref_xdivxsub(xi, 8, 9, range(512))
    part = xc.ref_xdivxsub(xi, 8, 9, [3, 511])
    assert part[0] == [whole[0][3], whole[0][511]] and part[1] == [whole[1][3], whole[1][511]]
    # LEv sums to 1 (the interpolant of the constant 1), whatever xi
    s = [sum(r[c] for r in xc.ref_lagrange(xi, 9, range(512))[0]) % P for c in range(3)]
    assert s == [1, 0, 0]


@pytest.mark.parametrize("name", sorted(xc.EV_LISTS))
@pytest.mark.parametrize("eb", xc.EV_EB)
def test_ref_evmap_matches_oracle(oracle, name, eb):
    case = xc.EvCase(xc.EV_LIST_N, eb, xc.EV_LISTS[name])
    assert case.n <= xc.PY_REF_MAX
    ref = xc.ref_evmap(case)
    assert ref.shape == (len(case.entries), 3)
    assert np.array_equal(ref, xc.oracle_evmap(oracle, case))
    # row blocks add up, in both references
    k = 200
    parts = xc.add_evals(xc.ref_evmap(case, 0, k), xc.ref_evmap(case, k))
    assert np.array_equal(parts, ref)
    assert np.array_equal(xc.add_evals(xc.oracle_evmap(oracle, case, 0, k), xc.oracle_evmap(oracle, case, k)), ref)


def test_oracle_evmap_reads_strided_rows(oracle):
    """oracle_evmap on the values equals oc_evmap on the device image (stride
    2^eb, its own leading dimension, the filler between the rows)"""
    import ctypes
    n, eb = 257, 2
    case = xc.EvCase(n, eb, xc.EV_SHAPE_ENTRIES)
    fill = np.uint64(0x0123456789ABCDEF)
    imgs = {poly: case.poly_image(poly, fill, 8) for poly in case.polys}
    n_ev = len(case.entries)
    pn = np.uint64(P)
    # row-major copies of the images: dim words per row, every row of the column present
    rows = {poly: np.ascontiguousarray((imgs[poly][:case.polys[poly].shape[0] * case.ld[poly]]
                                        .reshape(-1, case.ld[poly]) % pn).T) for poly in imgs}
    ptrs = (ctypes.c_void_p * n_ev)(*[rows[poly].ctypes.data for poly, _, _ in case.entries])
    strides = np.array([d for _, d, _ in case.entries], np.uint64)
    out = np.zeros((n_ev, 3), np.uint64)
    lev = np.ascontiguousarray((case.lev % pn).T)
    lpev = np.ascontiguousarray((case.lpev % pn).T)
    oracle.lib().oc_evmap(oracle._p(out), ctypes.cast(ptrs, ctypes.c_void_p), ctypes.c_void_p(strides.ctypes.data),
                          ctypes.c_void_p(case.dims.ctypes.data), ctypes.c_void_p(case.primes.ctypes.data), n_ev,
                          oracle._p(lev), oracle._p(lpev), n, eb)
    assert np.array_equal(out, xc.ref_evmap(case))
    for poly, img in imgs.items():
        dim, ld = case.polys[poly].shape[0], case.ld[poly]
        v = img[:dim * ld].reshape(dim, ld)
        assert np.array_equal(v[:, :xc.ev_span(n, eb):1 << eb], case.polys[poly])
        assert (v[:, xc.ev_span(n, eb):] == fill).all() and (v[:, 1::4] == fill).all() and (img[dim * ld:] == fill).all()
        assert ld >= xc.ev_span(n, eb)


@pytest.mark.parametrize("pol_bits,out_bits", [(pb, ob) for pb in range(0, 13) for ob in range(max(0, pb - 5), pb + 1)])
def test_fold_group_is_an_element_of_the_whole_fold(oracle, pol_bits, out_bits):
    rng = np.random.default_rng([pol_bits, out_bits])
    pol = xc.canonical(rng, 3 << pol_bits)
    sx = np.array(sc.f3(xc.lazy_ext(rng)), dtype=np.uint64)
    sinv = xc.fold_shift_inv(rng) % P
    whole = oracle.fri_fold(pol, pol_bits, out_bits, sx, sinv).reshape(-1, 3)
    rows = oracle.fri_get_transposed(pol, out_bits).reshape(1 << out_bits, -1)
    for g in sorted({0, (1 << out_bits) - 1, (1 << out_bits) // 3}):
        assert np.array_equal(oracle.fri_fold_group(rows[g], g, pol_bits, sx, sinv), whole[g]), g


# ------------------------------------------------------------------ shape lists
def test_lagrange_blocks_straddle_chunk_and_workgroup():
    n = 1 << xc.LAG_NBITS
    assert xc.LAG_BLOCKS == [(0, 1), (8191, 1), (5, 15), (16, 16), (3, 17), (0, 4096), (100, 4097), (4095, 4097),
                             (0, 8192), (8192, 0)]
    assert xc.LAG_BLOCKS == xc.row_blocks(n)
    sizes = {nr for _, nr in xc.LAG_BLOCKS}
    assert {xc.BI_CHUNK - 1, xc.BI_CHUNK, xc.BI_CHUNK + 1} <= sizes
    assert {xc.XDIV_WG_ROWS, xc.XDIV_WG_ROWS + 1} <= sizes and 0 in sizes and 1 in sizes
    assert xc.xdiv_threads(xc.XDIV_WG_ROWS) == 256 and xc.xdiv_threads(xc.XDIV_WG_ROWS + 1) == 512
    assert xc.xdiv_threads(1) == xc.xdiv_threads(17) == 256
    assert all(r0 + nr <= n for r0, nr in xc.LAG_BLOCKS)
    assert any(r0 + nr == n and nr > xc.XDIV_WG_ROWS and r0 for r0, nr in xc.LAG_BLOCKS)  # ends exactly at N
    assert any(r0 % xc.BI_CHUNK and nr % xc.BI_CHUNK for r0, nr in xc.LAG_BLOCKS)
    # every block but the two full ones leaves threads with rows on both sides of nrows (the unit denominators)
    full = [nr for _, nr in xc.LAG_BLOCKS if nr and nr == xc.xdiv_threads(nr) * xc.BI_CHUNK]
    assert full == [xc.XDIV_WG_ROWS, n]
    assert all(xc.xdiv_threads(nr) < nr < xc.xdiv_threads(nr) * xc.BI_CHUNK for nr in (4097,))
    assert xc.LAG_SMALL_NBITS == [0, 1, 4] and xc.LAG_BIG_NBITS == [24, 28]


def test_big_blocks_reach_the_high_twiddle_table():
    half = 1 << (xc.TW_LEVEL_BITS - 1)
    for n_bits in xc.LAG_BIG_NBITS:
        n = 1 << n_bits
        blocks = xc.big_blocks(n_bits)
        assert blocks == [(0, 33), (n - 100, 100), (n // 2 - 7, 50)]
        his = {xc.tw_index(r0 + k, n_bits)[1] for r0, nr in blocks for k in range(nr)}
        assert max(his) == (1 << xc.TW_LEVEL_BITS) - 1 and 0 in his      # the last entry and the first
        assert half - 1 in his and half in his                          # across the middle of the high table
        assert all(r0 + nr <= n for r0, nr in blocks)
    # up to 2^14 rows the low index is zero in every row: only a larger domain multiplies two table entries
    assert {xc.tw_index(k, 12)[0] for k in range(1 << 12)} == {0}
    assert {xc.tw_index(k, xc.LAG_NBITS)[0] for k in range(1 << xc.LAG_NBITS)} == {0}
    assert len({xc.tw_index(r, 28)[0] for r in range(40)}) == 40        # at 2^28 the low table moves row by row
    assert len({xc.tw_index(r, 24)[0] for r in range(40)}) == 40


def test_xdiv_rows_shapes():
    assert xc.XDIV_ROWS_BITS == [(8, 9), (11, 13), (10, 10)] and xc.XDIV_WHOLE_BITS == [(0, 1), (3, 4), (11, 13)]
    for nb, nbe in xc.XDIV_ROWS_BITS + xc.XDIV_WHOLE_BITS:
        assert nb <= nbe
    for _, nbe in xc.XDIV_ROWS_BITS:
        ne = 1 << nbe
        blocks = xc.row_blocks(ne)
        sizes = {nr for _, nr in blocks}
        assert {0, 1, xc.BI_CHUNK - 1, xc.BI_CHUNK, xc.BI_CHUNK + 1, ne // 2, ne // 2 + 1, ne} <= sizes
        assert all(r0 + nr <= ne for r0, nr in blocks) and any(r0 and r0 + nr == ne and nr > 1 for r0, nr in blocks)
    assert xc.xdiv_threads((1 << 12) + 1) > xc.XDIV_THREADS  # the (11, 13) domain's half plus one row
    assert [nbe for _, nbe in xc.XDIV_WHOLE_BITS] == [1, 4, 13]


def test_evmap_shapes_straddle_threads_iteration_and_block():
    assert xc.EV_N == [1, 255, 256, 257, 511, 513, 61439, 61440, 61441] and xc.EV_EB == [0, 2]
    ns = set(xc.EV_N)
    assert {xc.EV_THREADS - 1, xc.EV_THREADS, xc.EV_THREADS + 1} <= ns
    it = xc.EV_THREADS * xc.EV_UR
    assert it == 512 and {it - 1, it + 1} <= ns
    assert xc.EV_ROWS_PER_BLOCK == 61440 and {61439, 61440, 61441} <= ns
    assert xc.EV_LIST_N in ns and xc.EV_LIST_N > it and xc.EV_LIST_N <= xc.PY_REF_MAX
    n, k = xc.EV_SPLIT
    assert n == 61441 and 0 < k < n and k % xc.EV_THREADS and (n - k) % xc.EV_THREADS
    for n in xc.EV_N:
        lds = [xc.ev_col_ld(n, eb, e) for eb in xc.EV_EB for e in range(3)]
        assert len(set(lds)) == len(lds) and xc.ev_l_ld(n) == n + 7
        assert all(xc.ev_col_ld(n, eb, 0) >= xc.ev_span(n, eb) + 3 for eb in xc.EV_EB)
    # the largest case: ten columns of n << 2 words stay a few megabytes each
    assert 8 * xc.ev_col_ld(61441, 2, 45) < 2.1e6


def test_evmap_entry_lists_reach_every_grouping():
    g = {name: xc.ev_groups(entries) for name, entries in xc.EV_LISTS.items()}
    assert g["one_dim1"] == [(0, [(0, 0)])]
    assert len(g["four_same_prime"]) == 1 and len(g["four_same_prime"][0][1]) == xc.EV_GW
    assert [len(m) for _, m in g["five_same_prime"]] == [xc.EV_GW, 1]
    # the dim-3 entry's components lie in two groups
    assert [[e for e, _ in m] for _, m in g["dim3_straddles"]] == [[0, 1, 2, 2], [2, 3]]
    assert {p for p, _ in g["all_prime"]} == {1} and [len(m) for _, m in g["all_prime"]] == [4, 3]
    twice = xc.EV_LISTS["one_column_twice"]
    assert twice[0][0] == twice[1][0] and {twice[0][2], twice[1][2]} == {0, 1}
    assert twice[2][0] == twice[3][0] and twice[2][1] == 3 and {twice[2][2], twice[3][2]} == {0, 1}
    mixed = xc.EV_LISTS["mixed45"]
    assert len(mixed) == 45 and {d for _, d, _ in mixed} == {1, 3} and {p for _, _, p in mixed} == {0, 1}
    gm = g["mixed45"]
    assert [p for p, _ in gm] == sorted(p for p, _ in gm)                      # sorted by prime
    assert any(len({e for e, _ in m}) < len(m) and len(m) == xc.EV_GW for _, m in gm)
    assert sum(len(m) for _, m in gm) == sum(d for _, d, _ in mixed)
    assert any(len(m) < xc.EV_GW for _, m in gm)                               # a short last group
    assert g["empty"] == []
    # the list of the shape tests: a dim-3 entry across two groups under either prime
    assert [[e for e, _ in m] for _, m in g["shape"]] == [[0, 1, 2, 2], [2], [3, 3, 3, 4], [5]]
    assert set(xc.EV_LISTS) == {"one_dim1", "four_same_prime", "five_same_prime", "dim3_straddles", "all_prime",
                                "one_column_twice", "mixed45", "empty", "shape"}


def test_fold_shapes():
    assert xc.FOLD_WHOLE == [(0, 0), (1, 0), (3, 1), (3, 0), (5, 1), (5, 0), (13, 8), (14, 9), (9, 9)]
    small = [(pb, ob) for pb, ob in xc.FOLD_WHOLE if ob < 2]
    assert {pb - ob for pb, ob in small} == set(range(xc.FOLD_MAX_REDUCTION + 1))
    assert {ob for _, ob in small} == {0, 1}
    assert all(0 <= pb - ob <= xc.FOLD_MAX_REDUCTION for pb, ob in xc.FOLD_WHOLE)
    assert any((1 << ob) > xc.FOLD_THREADS for _, ob in xc.FOLD_WHOLE)          # more than one workgroup
    assert xc.FOLD_ROWS_BITS == [16, 24, 28] and xc.FOLD_ROWS_REDUCTION == [2, 5] and xc.FOLD_ROWS_NG == [1, 257]
    assert xc.FOLD_THREADS + 1 in xc.FOLD_ROWS_NG
    top = 0
    for pb in xc.FOLD_ROWS_BITS:
        for red in xc.FOLD_ROWS_REDUCTION:
            ob = pb - red
            for ng in xc.FOLD_ROWS_NG:
                g0s = xc.fold_rows_g0(pb, ob, ng)
                assert g0s[0] == 0 and g0s[1] + ng == 1 << ob and len(set(g0s)) == 3
                seam = g0s[2]
                assert 0 < seam and seam + ng <= 1 << ob
                lo0, hi0 = xc.fold_tw_index(seam, pb)
                lo1, hi1 = xc.fold_tw_index(seam + ng - 1, pb)
                if ng > 1:
                    assert hi1 > hi0 > 0                                        # the high index steps inside the block
                else:
                    assert lo0 == 0 and hi0 > 0                                 # the group on the seam itself
                top = max(top, xc.fold_tw_index(g0s[1] + ng - 1, pb)[1])
                # the rows of a block stay tiny whatever pol_bits
                assert ng * (3 << red) * 8 < 1 << 20
    assert top == (1 << (xc.TW_LEVEL_BITS - 2)) - 1   # reduction 2: the last entry of the high table's first quarter
    # the whole folds up to 2^20 -> 2^16 stop at high index 2^10 - 1
    assert xc.fold_tw_index((1 << 16) - 1, 20)[1] == (1 << 10) - 1


def test_transpose_and_opening_shapes():
    assert xc.FRI_TRANSPOSE == [(1, 0), (8, 0), (8, 3), (4096, 1), (4096, 11), (96, 5), (257 * 4, 2)]
    for degree, tbits in xc.FRI_TRANSPOSE:
        assert degree % (1 << tbits) == 0
    wh = [(1 << tb, d >> tb) for d, tb in xc.FRI_TRANSPOSE]
    assert any(w == 1 for w, _ in wh) and any(h == 1 and w > 1 for w, h in wh)
    assert any(w > h > 1 for w, h in wh) and any(h > w > 1 for w, h in wh)
    assert any(d % 256 and d > 256 for d, _ in xc.FRI_TRANSPOSE)                # a ragged last workgroup
    assert xc.OPEN_NROWS == [1, 2, 4, 1024] and xc.OPEN_NCOLS == [0, 1, 4, 63, 64, 65, 130] and xc.OPEN_NQ == [1, 300]
    assert {xc.OPEN_THREADS - 1, xc.OPEN_THREADS, xc.OPEN_THREADS + 1} <= set(xc.OPEN_NCOLS)
    assert max(xc.OPEN_NCOLS) > 2 * xc.OPEN_THREADS
    rng = np.random.default_rng(1)
    for nrows in xc.OPEN_NROWS:
        for nq in xc.OPEN_NQ:
            idx = xc.open_indices(nrows, nq, rng)
            assert idx.shape == (nq,) and idx.dtype == np.uint64 and int(idx.max()) == nrows - 1
            if nq > 1:
                assert 0 in idx and len(set(idx.tolist())) < nq
                assert nrows == 1 or list(idx) != sorted(idx)
