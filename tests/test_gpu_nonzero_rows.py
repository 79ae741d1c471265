"""zkgpu_nonzero_rows_dev (csrc/stark.hip k_nz_count / k_nz_emit) against numpy:
the count of the rows of a column-major section that are not zero mod p and
the lowest max_rows of them, ascending.  Sizes around the wave (64), the
workgroup's pass (256) and the counted block (1024), one above 2^16; the rows
in [n, ld) hold nonzero words that must not be seen; the output's words past
1 + max_rows hold a sentinel that must survive."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 0xFFFFFFFF00000001
NONE = 2**64 - 1
SENT = np.uint64(0xA5C3A5C3F00DFACE)
FILL = np.uint64(0x0123456789ABCDEF)  # rows [n, ld): nonzero
GUARD = 8
SIZES = [1, 63, 64, 65, 255, 256, 257, 4097, 2**16 + 3]
MAX_ROWS = [0, 1, 16, 4096]


def expected(cols, max_rows):
    rows = np.flatnonzero((cols % np.uint64(P) != 0).any(axis=0)).astype(np.uint64)
    out = np.full(1 + max_rows + GUARD, SENT, np.uint64)
    out[0] = rows.size
    out[1:1 + max_rows] = NONE
    k = min(rows.size, max_rows)
    out[1:1 + k] = rows[:k]
    return out


def run(zkgpu, cols, max_rows):
    ncols, n = cols.shape
    ld = n + 5
    img = np.full(ncols * ld + GUARD, FILL, np.uint64)
    img[:ncols * ld].reshape(ncols, ld)[:, :n] = cols
    d_in = zkgpu.to_device(img)
    d_out = zkgpu.to_device(np.full(1 + max_rows + GUARD, SENT, np.uint64))
    zkgpu.nonzero_rows_dev(d_out, d_in, ld, ncols, n, max_rows)
    zkgpu.synchronize()
    return zkgpu.from_device(d_out)


def patterns(n, ncols, max_rows):
    """name -> (ncols, n) words"""
    rng = np.random.default_rng(1000 * n + ncols)
    z = np.zeros((ncols, n), np.uint64)
    out = {"all_zero": z}
    a = z.copy()
    a[0, n - 1] = 1
    out["last_row"] = a
    a = z.copy()
    a[ncols - 1, ::7] = 3
    out["last_column"] = a
    # the value p is zero; p + 1 and 2^64 - 1 are not
    a = np.full((ncols, n), P, np.uint64)
    a[rng.integers(ncols), n // 2] = P + 1
    a[rng.integers(ncols), 0] = NONE
    out["lazy_words"] = a
    for name, k in (("exactly_max_rows", max_rows), ("max_rows_plus_one", max_rows + 1)):
        if 0 < k <= n:
            a = z.copy()
            hit = rng.choice(n, k, replace=False)
            a[rng.integers(ncols, size=k), hit] = rng.integers(1, P, k, dtype=np.uint64)
            out[name] = a
    out["every_row"] = rng.integers(1, P, (ncols, n), dtype=np.uint64)
    a = z.copy()  # both sides of every 64-row boundary (256 and 1024 among them)
    b = np.arange(64, n, 64)
    a[rng.integers(ncols, size=b.size), b] = 5
    a[rng.integers(ncols, size=b.size), b - 1] = P - 1
    out["block_boundaries"] = a
    return out


@pytest.mark.parametrize("ncols", [1, 3, 7])
@pytest.mark.parametrize("n", SIZES)
def test_vs_numpy(zkgpu, n, ncols):
    for max_rows in MAX_ROWS:
        for name, cols in patterns(n, ncols, max_rows).items():
            got = run(zkgpu, cols, max_rows)
            want = expected(cols, max_rows)
            assert np.array_equal(got, want), (name, max_rows, got[:8], want[:8])


def test_result_does_not_depend_on_where_the_hits_lie(zkgpu):
    """the same hits in another column give the same rows (3 columns, 4097 rows)"""
    rng = np.random.default_rng(5)
    hit = np.sort(rng.choice(4097, 40, replace=False))
    outs = []
    for c in range(3):
        a = np.zeros((3, 4097), np.uint64)
        a[c, hit] = 9
        outs.append(run(zkgpu, a, 16))
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    assert outs[0][0] == 40 and np.array_equal(outs[0][1:17], hit[:16].astype(np.uint64))


def test_empty_shapes_write_count_zero(zkgpu):
    for n, ncols in ((0, 3), (100, 0), (0, 0)):
        d_in = zkgpu.to_device(np.full(1024, FILL, np.uint64))
        d_out = zkgpu.to_device(np.full(1 + 16 + GUARD, SENT, np.uint64))
        zkgpu.nonzero_rows_dev(d_out, d_in, 128, ncols, n, 16)
        zkgpu.synchronize()
        want = np.full(1 + 16 + GUARD, SENT, np.uint64)
        want[0] = 0
        want[1:17] = NONE
        assert np.array_equal(zkgpu.from_device(d_out), want)


def test_refusals(zkgpu):
    d_in = zkgpu.to_device(np.zeros(1024, np.uint64))
    d_out = zkgpu.to_device(np.full(4200, SENT, np.uint64))
    for args, message in (((d_out, d_in, 99, 3, 100, 16), "nonzero_rows: ld < n"),
                          ((d_out, d_in, 100, 3, 100, 4097), "nonzero_rows: max_rows 4097 > 4096"),
                          ((None, d_in, 100, 3, 100, 16), "nonzero_rows: null pointer"),
                          ((d_out, None, 100, 3, 100, 16), "nonzero_rows: null pointer")):
        with pytest.raises(zkgpu.ZkgpuError) as e:
            zkgpu.nonzero_rows_dev(*args)
        assert str(e.value) == "zkgpu_nonzero_rows_dev failed (-2): " + message
    zkgpu.synchronize()
    assert np.array_equal(zkgpu.from_device(d_out), np.full(4200, SENT, np.uint64))  # nothing was queued
