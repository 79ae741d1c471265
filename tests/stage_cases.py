"""Shapes, inputs and Python-integer references of the stage primitives.

The kernels behind the prover's stage steps (csrc/stark.hip: the tiled grand
product k_z_ratio / k_z_totals / k_z_apply, k_ext_powers, k_qsplit,
k_cols3_to_interleaved, k_copy_rows, k_rand_cols; csrc/ntt.hip: the 32 x 32
tile transposes) change path with the row count: thread runs of Z_PER rows,
waves, SCAN_THREADS, Z_TILE, more than SCAN_THREADS tiles, a grid-dependent
power step, ragged transpose tiles.  This module names the sizes at which
each path changes, builds inputs (canonical words, and "lazy" words: the same
field elements written as x + p wherever that fits in 64 bits, among them the
words p, p + 1 and 2^64 - 1), and restates each operation in Python integers.
tests/test_stage_cases.py checks all of it on the CPU against the oracle;
tests/test_gpu_stage_primitives.py runs the kernels against it.

Arrays are "columns": numpy uint64 of shape (ncols, n), row k of column c at
[c, k] (the device layout with ld = n); an F_p^3 column is three of them.
"""
import numpy as np

from zkgpu.synthetic import rand_u64

P = 0xFFFFFFFF00000001
EPS = 0xFFFFFFFF  # 2^64 - p: x + p < 2^64 iff x < EPS
M64 = (1 << 64) - 1

# csrc/stark.hip
Z_PER = 4
SCAN_THREADS = 256
Z_TILE = Z_PER * SCAN_THREADS
EXT_ROWS_PER_THREAD = 64   # ext_powers: threads = ceil(n / 64), 256 per block
BLOCK = 256
TR_TILE = 32               # csrc/ntt.hip k_rows_to_cols / k_cols_to_rows
WAVE = 64


# ------------------------------------------------------------------ shape lists
# thread-run (4), wave (64 x 4 = 256), SCAN_THREADS and tile (1024) edges;
# 257 tiles: k_z_totals walks 2 totals per thread, thread 128 holds one tile
# and threads 129..255 none; 513 tiles less 7 rows: 3 per thread, ragged tail
Z_N = [1, 2, 3, 4, 5, 255, 256, 257, 511, 513, 1023, 1024, 1025, 2051, 5 * 1024 - 1, 256 * 1024 + 1,
       513 * 1024 - 7]
Z_BLOCK_N = [1, 5, 257, 1025, 2051, 5 * 1024 - 1, 256 * 1024 + 1, 513 * 1024 - 7]
Z_MANY_N = [257, 2051]
Z_STALE_SEQUENCE = [513 * 1024 - 7, 5, 1025]  # a long call, then short ones on its scratch
Z0_LAZY = (P + 5, M64, P)                      # == (5, 2^32 - 2, 0): neither the unit nor canonical
PY_REF_MAX = 2048                              # the Python-integer reference runs up to here

EXT_POWERS_N = [1, 2, 255, 256, 257, 16384, 16385, 50001]
QSPLIT_N = [1, 255, 257, 1000]
QSPLIT_QDEG = [1, 2, 3, 4]
QSPLIT_DIM_STRIDE = [(3, 3), (1, 3), (2, 5)]
COLS3_N = [1, 255, 257, 4097]
TRANSPOSE_SHAPES = [(1, 1), (31, 33), (32, 32), (33, 31), (1, 100), (1000, 1), (257, 65)]
COPY_NROWS = [1, 63, 64, 65, 257]
RAND_NROWS = [1, 255, 257]
RAND_LOG_N = 9


def z_lds(n):
    """(z_ld, num_ld, den_ld): all different, all above n"""
    return n + 3, n + 64, n + 1


def z_tiles(n):
    return (n + Z_TILE - 1) // Z_TILE


def z_totals_runs(n):
    """k_z_totals: (tiles per thread, [tiles held by thread t])"""
    nt = z_tiles(n)
    per = (nt + SCAN_THREADS - 1) // SCAN_THREADS
    return per, [max(0, min(nt, (t + 1) * per) - t * per) for t in range(SCAN_THREADS)]


def ext_powers_blocks(n):
    threads = (n + EXT_ROWS_PER_THREAD - 1) // EXT_ROWS_PER_THREAD
    return (threads + BLOCK - 1) // BLOCK


def copy_wrap(nrows):
    """(src_log_mod, src_row0, src_ld) of a window that crosses 2^src_log_mod"""
    log_mod = max(1, (nrows - 1).bit_length())
    row0 = (1 << log_mod) - nrows // 2 if nrows > 1 else 1 << log_mod
    return log_mod, row0, (1 << log_mod) + 4


def rand_block_row0(nrows):
    """row0 of a block whose rows cross 2^RAND_LOG_N"""
    n = 1 << RAND_LOG_N
    return n - nrows // 2 if nrows > 1 else n


# ------------------------------------------------------------------ F_p, F_p^3
def f3(a):
    return tuple(int(v) % P for v in a)


ONE3 = (1, 0, 0)


def f3_mul(a, b):
    """(a0 + a1 x + a2 x^2)(b0 + b1 x + b2 x^2) with x^3 = x + 1 (x^4 = x^2 + x)"""
    a0, a1, a2 = a
    b0, b1, b2 = b
    c0 = a0 * b0
    c1 = a0 * b1 + a1 * b0
    c2 = a0 * b2 + a1 * b1 + a2 * b0
    c3 = a1 * b2 + a2 * b1
    c4 = a2 * b2
    return ((c0 + c3) % P, (c1 + c3 + c4) % P, (c2 + c4) % P)


def f3_inv(a):
    """b with a b = 1: the first column of the inverse of the matrix of
    "multiply by a" (columns a, a x, a x^2), by Cramer's rule; checked"""
    a0, a1, a2 = a
    m = [[a0, a2, a1], [a1, a0 + a2, a1 + a2], [a2, a1, a0 + a2]]
    cof = [m[1][1] * m[2][2] - m[1][2] * m[2][1],
           m[1][2] * m[2][0] - m[1][0] * m[2][2],
           m[1][0] * m[2][1] - m[1][1] * m[2][0]]
    det = (m[0][0] * cof[0] + m[0][1] * cof[1] + m[0][2] * cof[2]) % P
    if det == 0:
        raise ZeroDivisionError("f3_inv(0)")
    di = pow(det, -1, P)
    # adj(M)[i][0] = cofactor of m[0][i]
    b = (cof[0] * di % P, cof[1] * di % P, cof[2] * di % P)
    assert f3_mul(f3(a), b) == ONE3
    return b


def rows3(cols):
    """(3, n) columns -> list of n reduced 3-tuples of Python integers"""
    c = [[int(v) % P for v in col] for col in cols]
    return list(zip(*c))


def cols3(rows):
    """list of 3-tuples -> (3, n) uint64 columns"""
    return np.array(rows, dtype=np.uint64).reshape(-1, 3).T.copy()


# ------------------------------------------------------------------ references
def ref_calculate_z(num, den, z0=ONE3):
    """z[k] = z0 prod_{i<k} num[i] / den[i] and the total z0 prod_{i<n}
    (Polinomial::calculateZ with a block's z0); num, den: lists of 3-tuples.
    One inversion for the whole array (Montgomery's trick)."""
    n = len(num)
    z0 = f3(z0)
    if n == 0:
        return [], z0
    pre = [den[0]]
    for k in range(1, n):
        pre.append(f3_mul(pre[-1], den[k]))
    inv = f3_inv(pre[-1])
    dinv = [None] * n
    for k in range(n - 1, 0, -1):
        dinv[k] = f3_mul(inv, pre[k - 1])
        inv = f3_mul(inv, den[k])
    dinv[0] = inv
    z, run = [], z0
    for k in range(n):
        z.append(run)
        run = f3_mul(run, f3_mul(num[k], dinv[k]))
    return z, run


def ref_powers3(base, n):
    out, r, b = [], ONE3, f3(base)
    for _ in range(n):
        out.append(r)
        r = f3_mul(r, b)
    return out


def ref_qsplit(qq1, n, q_deg, shift_in, dim, stride):
    """{output column stride * p + d: [qq1[d][p n + k] * shift_in^p for k < n]}, d < dim, p < q_deg"""
    out, f = {}, 1
    for p in range(q_deg):
        for d in range(dim):
            out[stride * p + d] = [int(qq1[d][p * n + k]) % P * f % P for k in range(n)]
        f = f * (int(shift_in) % P) % P
    return out


def ref_copy_rows(dst, dst_row0, dst_cols, src, src_row0, src_log_mod, src_cols, ncols, nrows):
    """in place on dst (columns x dst_ld) from src (columns x src_ld), words as they are"""
    for k in range(ncols):
        dc = k if dst_cols is None else dst_cols[k]
        sc = k if src_cols is None else src_cols[k]
        for j in range(nrows):
            r = src_row0 + j
            if src_log_mod:
                r %= 1 << src_log_mod
            dst[dc][dst_row0 + j] = src[sc][r]


def ref_rand_cols(dst, cols, row0, nrows, log_n, seed, stream):
    """in place on dst (columns x ld): local row r = global row (row0 + r) mod 2^log_n (no wrap: log_n None)"""
    for c in cols:
        for r in range(nrows):
            g = row0 + r
            if log_n is not None:
                g %= 1 << log_n
            dst[c][r] = rand_u64(seed, stream, c, g)


# ------------------------------------------------------------------ oracle forms
def oracle_calculate_z(oc, num, den, z0=None):
    """The oracle's calculateZ on (3, n) columns reduced mod p -> ((3, n) z,
    total 3-tuple, closes).  A z0 is a row (z0, 1) put in front (every later
    z picks up the factor); a row (1, 1) behind makes the last z the total."""
    n = num.shape[1]
    pn = np.uint64(P)
    head = np.array([f3(z0 if z0 is not None else ONE3)], dtype=np.uint64)
    one = np.array([ONE3], dtype=np.uint64)
    nr = np.ascontiguousarray(np.concatenate([head, (num % pn).T, one]))
    dr = np.ascontiguousarray(np.concatenate([one, (den % pn).T, one]))
    z = np.zeros((n + 2, 3), np.uint64)
    oc.lib().oc_calculate_z(oc._p(z), 3, oc._p(nr), 3, oc._p(dr), 3, n + 2)
    total = tuple(int(v) for v in z[n + 1])
    return np.ascontiguousarray(z[1:n + 1].T), total, total == tuple(head[0])


def oracle_powers3(oc, base, n):
    out = np.zeros((n, 3), np.uint64)
    oc.lib().oc_powers3(oc._p(out), oc._p(np.array(f3(base), dtype=np.uint64)), n)
    return np.ascontiguousarray(out.T)


# ------------------------------------------------------------------ inputs
SPECIAL_RESIDUES = [0, 1, EPS - 1]  # lazy(): the words p, p + 1, 2^64 - 1


def canonical(rng, shape, special=True):
    """random canonical words; a quarter below EPS (where x + p still fits a
    word), and, given six words or more, the three residues whose lazy words
    are p, p + 1 and 2^64 - 1"""
    x = rng.integers(0, P, size=shape, dtype=np.uint64)
    small = rng.random(shape) < 0.25
    x[small] = rng.integers(0, EPS, size=int(small.sum()), dtype=np.uint64)
    if special and x.size >= 6:
        at = rng.choice(x.size, size=len(SPECIAL_RESIDUES), replace=False)
        x.reshape(-1)[at] = np.array(SPECIAL_RESIDUES, dtype=np.uint64)
    return x


def lazy(x):
    """the same field elements, p added wherever the word stays below 2^64"""
    x = np.asarray(x, dtype=np.uint64)
    return np.where(x < np.uint64(EPS), x + np.uint64(P), x)


def nonzero_rows(cols):
    """every row of a (3, n) F_p^3 column is a non-zero field element"""
    return bool(np.all((cols % np.uint64(P)).any(axis=0)))


class ZCase:
    """A grand product over n rows that closes (den = num one row on), its
    lazy form, and two products one denominator word away from it (last row,
    row 0) that do not close."""

    def __init__(self, n, seed=0):
        rng = np.random.default_rng([n, seed])
        self.n = n
        self.num = canonical(rng, (3, n))
        while not nonzero_rows(self.num):  # (a row of three zero words: 2^-192 each)
            self.num = canonical(rng, (3, n))
        self.den = np.roll(self.num, -1, axis=1)
        self.num_lazy, self.den_lazy = lazy(self.num), lazy(self.den)
        self.den_bad_last = self._bump(self.den, n - 1)
        self.den_bad_first = self._bump(self.den, 0)

    @staticmethod
    def _bump(den, row):
        d = den.copy()
        d[0, row] = (int(d[0, row]) + 1) % P
        if not d[:, row].any():  # (1 - 1, 0, 0): step over zero
            d[0, row] = 1
        return d

    def dens(self):
        return {"closing": self.den, "lazy": self.den_lazy, "bad_last": self.den_bad_last,
                "bad_first": self.den_bad_first}


class ZBlockCase:
    """An arbitrary (not closing) product: independent num and den, lazy words."""

    def __init__(self, n, seed=1):
        rng = np.random.default_rng([n, seed])
        self.n = n
        self.num = lazy(canonical(rng, (3, n)))
        self.den = lazy(canonical(rng, (3, n)))
        while not nonzero_rows(self.den):
            self.den = lazy(canonical(rng, (3, n)))


def ext_bases(rng):
    """name -> base of zkgpu_ext_powers_dev"""
    r = [int(v) for v in rng.integers(0, P, size=3, dtype=np.uint64)]
    return {"random": tuple(r), "base_field": (r[0], 0, 0), "zero": (0, 0, 0), "one": (1, 0, 0),
            "lazy": (P + 3, M64, r[2] % EPS + P)}
