"""CPU checks of tests/stage_cases.py: the Python-integer references equal the
oracle, every shape list reaches the kernel path it is there for, and no
grand-product case has a zero denominator (out of scope: the reference
inverts the whole column at once, the GPU per thread, and they differ there
by design -- so the inputs must never contain one)."""
import numpy as np
import pytest

import stage_cases as sc

P = sc.P


# ------------------------------------------------------------------ references vs the oracle
def test_f3_mul_and_inv_match_oracle(oracle):
    rng = np.random.default_rng(1)
    edge = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (P - 1, P - 1, P - 1), (P - 1, 0, 1), (sc.EPS, sc.EPS - 1, 1)]
    vals = edge + [tuple(int(v) for v in rng.integers(0, P, size=3, dtype=np.uint64)) for _ in range(60)]
    for a in vals:
        for b in vals[:12]:
            assert sc.f3_mul(a, b) == tuple(int(v) for v in oracle.gl3_mul(np.array(a, np.uint64),
                                                                        np.array(b, np.uint64))), (a, b)
        if any(a):
            assert sc.f3_inv(a) == tuple(int(v) for v in oracle.gl3_inv(np.array(a, np.uint64))), a
    with pytest.raises(ZeroDivisionError):
        sc.f3_inv((0, 0, 0))


@pytest.mark.parametrize("n", [n for n in sc.Z_N if n <= sc.PY_REF_MAX])
def test_ref_calculate_z_matches_oracle(oracle, n):
    """z0 = 1: oc_calculate_z itself, for every denominator of the case"""
    case = sc.ZCase(n)
    num = np.ascontiguousarray(case.num.T)
    for name, den in case.dens().items():
        zo = np.zeros((n, 3), np.uint64)
        closes = oracle.lib().oc_calculate_z(oracle._p(zo), 3, oracle._p(num), 3,
                                             oracle._p(np.ascontiguousarray((den % np.uint64(P)).T)), 3, n)
        z, total = sc.ref_calculate_z(sc.rows3(case.num), sc.rows3(den))
        assert z == [tuple(int(v) for v in r) for r in zo], name
        assert (total == sc.ONE3) == bool(closes) == (name in ("closing", "lazy")), name
        # the same through the oracle form the GPU test uses (rows put before and behind)
        z2, total2, closes2 = sc.oracle_calculate_z(oracle, case.num, den)
        assert np.array_equal(z2.T, zo) and total2 == total and closes2 == bool(closes), name


@pytest.mark.parametrize("n", [n for n in sc.Z_BLOCK_N if n <= sc.PY_REF_MAX])
def test_ref_calculate_z_with_z0_matches_oracle(oracle, n):
    case = sc.ZBlockCase(n)
    z, total = sc.ref_calculate_z(sc.rows3(case.num), sc.rows3(case.den), sc.Z0_LAZY)
    zo, to, closes = sc.oracle_calculate_z(oracle, case.num, case.den, sc.Z0_LAZY)
    assert np.array_equal(sc.cols3(z), zo) and total == to and not closes
    # z0 times the z0 = 1 product, row by row
    z1, t1 = sc.ref_calculate_z(sc.rows3(case.num), sc.rows3(case.den))
    z0 = sc.f3(sc.Z0_LAZY)
    assert z0 == (5, 2**32 - 2, 0)
    assert z == [sc.f3_mul(z0, r) for r in z1] and total == sc.f3_mul(z0, t1)


def test_ref_calculate_z_empty():
    assert sc.ref_calculate_z([], [], sc.Z0_LAZY) == ([], (5, 2**32 - 2, 0))


@pytest.mark.parametrize("n", [n for n in sc.EXT_POWERS_N if n <= sc.PY_REF_MAX])
def test_ref_powers3_matches_oracle(oracle, n):
    for name, base in sc.ext_bases(np.random.default_rng(n)).items():
        assert np.array_equal(sc.cols3(sc.ref_powers3(base, n)), sc.oracle_powers3(oracle, base, n)), name
    if n > 1:
        zero = sc.ref_powers3((0, 0, 0), n)
        assert zero[0] == sc.ONE3 and set(zero[1:]) == {(0, 0, 0)}


def test_ref_qsplit_matches_oracle_products(oracle):
    rng = np.random.default_rng(2)
    n, q_deg, shift = 5, 3, P + 7
    qq1 = sc.lazy(sc.canonical(rng, (2, q_deg * n + 3)))
    got = sc.ref_qsplit(qq1, n, q_deg, shift, 2, 5)
    assert sorted(got) == [0, 1, 5, 6, 10, 11]
    for p in range(q_deg):
        f = oracle.gl_pow(7, p)
        for d in range(2):
            assert got[5 * p + d] == [oracle.gl_mul(int(qq1[d, p * n + k]) % P, f) for k in range(n)]


def test_ref_copy_rows_and_rand_cols(oracle):
    rng = np.random.default_rng(3)
    src = rng.integers(0, sc.M64, size=(3, 20), dtype=np.uint64)
    dst = np.zeros((5, 12), np.uint64)
    sc.ref_copy_rows(dst, 2, [3, 0, 2], src, 14, 4, [1, 1, 0], 3, 6)
    rows = (14 + np.arange(6)) % 16
    exp = np.zeros((5, 12), np.uint64)
    exp[3, 2:8], exp[0, 2:8], exp[2, 2:8] = src[1, rows], src[1, rows], src[0, rows]
    assert np.array_equal(dst, exp)
    dst[:] = 0
    sc.ref_copy_rows(dst, 0, None, src, 3, 0, None, 2, 5)
    assert np.array_equal(dst[:2, :5], src[:2, 3:8]) and not dst[2:].any() and not dst[:, 5:].any()
    out = np.zeros((6, 8), np.uint64)
    sc.ref_rand_cols(out, [5, 0, 3], 510, 6, 9, 77, 1)
    for c in (5, 0, 3):
        assert [int(v) for v in out[c, :6]] == [oracle.lib().oc_rand_u64(77, 1, c, (510 + r) % 512) for r in range(6)]
    assert not out[[1, 2, 4]].any() and not out[:, 6:].any()


# ------------------------------------------------------------------ inputs
def test_lazy_words():
    rng = np.random.default_rng(4)
    x = sc.canonical(rng, (3, 500))
    y = sc.lazy(x)
    assert x.max() < P and np.array_equal(y % np.uint64(P), x)
    # p is added exactly where the sum still fits a word
    assert np.array_equal(y != x, x < np.uint64(sc.EPS)) and (y != x).sum() > 300
    assert {P, P + 1, sc.M64} <= set(int(v) for v in y.reshape(-1))
    assert [int(v) % P for v in sc.Z0_LAZY] == [5, 2**32 - 2, 0] and min(sc.Z0_LAZY) >= P


@pytest.mark.parametrize("n", sc.Z_N)
def test_no_zero_denominator_closing(n):
    case = sc.ZCase(n)
    assert sc.nonzero_rows(case.num)
    for name, den in case.dens().items():
        assert den.shape == (3, n) and sc.nonzero_rows(den), name
    assert np.array_equal(case.den_lazy % np.uint64(P), case.den)
    for bad, row in ((case.den_bad_last, n - 1), (case.den_bad_first, 0)):
        diff = np.argwhere(bad != case.den)
        assert diff.tolist() == [[0, row]]  # one word, and another field element (both canonical)
        assert bad.max() < P


@pytest.mark.parametrize("n", sc.Z_BLOCK_N)
def test_no_zero_denominator_block(n):
    case = sc.ZBlockCase(n)
    assert sc.nonzero_rows(case.den) and case.den.shape == case.num.shape == (3, n)
    assert (case.den >= np.uint64(P)).any() or n < 3


# ------------------------------------------------------------------ shape lists
def test_z_shapes_reach_every_path():
    ns = sc.Z_N
    assert ns == [1, 2, 3, 4, 5, 255, 256, 257, 511, 513, 1023, 1024, 1025, 2051, 5 * 1024 - 1, 256 * 1024 + 1,
                  513 * 1024 - 7]
    for n in ns:
        lds = sc.z_lds(n)
        assert len(set(lds)) == 3 and min(lds) > n
    assert any(n % sc.Z_PER for n in ns) and any(n % sc.Z_TILE for n in ns if n > sc.Z_TILE)
    assert {sc.Z_PER - 1, sc.Z_PER, sc.Z_PER + 1} <= set(ns)                      # a thread's run
    assert {sc.SCAN_THREADS - 1, sc.SCAN_THREADS, sc.SCAN_THREADS + 1} <= set(ns)  # the first strided pass
    assert {sc.Z_TILE - 1, sc.Z_TILE, sc.Z_TILE + 1} <= set(ns)                   # a tile
    assert all(sc.z_totals_runs(n)[0] == 1 for n in ns if n <= 256 * 1024)
    # 257 tiles: two per thread, thread 128 holds a single tile, 127 threads none
    per, runs = sc.z_totals_runs(256 * 1024 + 1)
    assert sc.z_tiles(256 * 1024 + 1) == 257 and per == 2
    assert runs[:128] == [2] * 128 and runs[128] == 1 and runs[129:] == [0] * 127
    # 513 tiles: three per thread, the last tile 7 rows short
    n = 513 * 1024 - 7
    per, runs = sc.z_totals_runs(n)
    assert sc.z_tiles(n) == 513 and per == 3 and n % sc.Z_TILE == sc.Z_TILE - 7 and sum(runs) == 513
    # the largest case: three extension columns under 40 MB
    assert 3 * 3 * 8 * max(sc.z_lds(n)) < 40e6
    assert set(sc.Z_BLOCK_N) <= set(ns) and {256 * 1024 + 1, n} <= set(sc.Z_BLOCK_N)
    assert any(sc.z_tiles(m) > 1 for m in sc.Z_BLOCK_N if m <= sc.PY_REF_MAX)
    seq = sc.Z_STALE_SEQUENCE
    assert seq == [513 * 1024 - 7, 5, 1025] and seq[0] > seq[2] > seq[1]
    assert sc.z_tiles(seq[2]) == 2  # the short layout's tile totals lie inside the long call's ratio words


def test_other_shapes_reach_every_path():
    assert sc.EXT_POWERS_N == [1, 2, 255, 256, 257, 16384, 16385, 50001]
    assert [sc.ext_powers_blocks(n) for n in (16384, 16385, 50001)] == [1, 2, 4]
    assert any(n > sc.BLOCK for n in sc.EXT_POWERS_N if sc.ext_powers_blocks(n) == 1)  # a thread steps by base^T
    assert sc.QSPLIT_N == [1, 255, 257, 1000] and sc.QSPLIT_QDEG == [1, 2, 3, 4]
    assert (1, 3) in sc.QSPLIT_DIM_STRIDE and (2, 5) in sc.QSPLIT_DIM_STRIDE
    assert sc.COLS3_N == [1, 255, 257, 4097]
    assert sc.TRANSPOSE_SHAPES == [(1, 1), (31, 33), (32, 32), (33, 31), (1, 100), (1000, 1), (257, 65)]
    t = sc.TR_TILE
    assert any(r % t and c % t and r > t and c > t for r, c in sc.TRANSPOSE_SHAPES)  # ragged both ways
    assert sc.COPY_NROWS == [1, 63, 64, 65, 257] and {sc.WAVE - 1, sc.WAVE, sc.WAVE + 1} <= set(sc.COPY_NROWS)
    for nrows in sc.COPY_NROWS:
        log_mod, row0, ld = sc.copy_wrap(nrows)
        m = 1 << log_mod
        assert log_mod >= 1 and m <= ld and row0 + nrows > m  # the window crosses 2^log_mod
        assert nrows == 1 or row0 < m
    assert sc.RAND_NROWS == [1, 255, 257]
    for nrows in sc.RAND_NROWS:
        assert sc.rand_block_row0(nrows) + nrows > 1 << sc.RAND_LOG_N
