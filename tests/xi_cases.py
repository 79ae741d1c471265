"""Shapes, inputs and Python-integer references of the evaluation, FRI and
opening primitives.

csrc/stark.hip k_xdiv_rows (zkgpu_lagrange_xi_rows_dev, zkgpu_xdivxsub_dev,
zkgpu_xdivxsub_rows_dev), k_evmap_groups / k_evmap_sum_subs (zkgpu_evmap_dev
and its host-side grouping in csrc/api.hip), csrc/fri.hip k_fri_fold /
k_fri_transpose and csrc/poseidon.hip k_merkle_open change path with the row
count, the row block's place in the domain and the entry list.  This module
names the sizes at which they do, builds the inputs (lazy words as in
stage_cases) and restates LEv / LpEv, xDivXSub and evmap in Python integers.
tests/test_xi_cases.py checks all of it on the CPU against the oracle;
tests/test_gpu_xi_primitives.py runs the kernels against it.

Host-only: no GPU, no torch.
"""
import ctypes

import numpy as np

from stage_cases import EPS, M64, ONE3, P, PY_REF_MAX, canonical, f3, f3_inv, f3_mul, lazy, rows3  # noqa: F401

# csrc/stark.hip k_xdiv_rows
BI_CHUNK = 16                       # rows of one thread: they share one inversion
XDIV_THREADS = 256
XDIV_WG_ROWS = BI_CHUNK * XDIV_THREADS  # 4096: one more row doubles the thread count T
TW_MAX_LOG = 28                     # csrc/gl_host.hpp: twiddles omega_{2^28}^e = lo[e mod 2^14] * hi[e >> 14]
TW_LEVEL_BITS = 14
# csrc/stark.hip k_evmap_groups, csrc/api.hip zkgpu_evmap_dev
EV_THREADS = 256
EV_UR = 2                           # rows per thread and iteration
EV_GW = 4                           # sub-entries per group
EV_ROWS_PER_THREAD = 240
EV_ROWS_PER_BLOCK = EV_ROWS_PER_THREAD * EV_THREADS  # 61440 = evmap_rows_per_block()
# csrc/fri.hip, csrc/poseidon.hip
FOLD_THREADS = 256
FOLD_MAX_REDUCTION = 5
OPEN_THREADS = 64                   # k_merkle_open: one workgroup per query loops over the columns


# ------------------------------------------------------------------ field helpers
GL_W32 = 7277203076849721926        # Goldilocks::W[32], of order 2^32


def gl_w(n_bits):
    """Goldilocks::w(n_bits): the library's root of unity of order 2^n_bits, W[32]^(2^(32 - n_bits))"""
    return pow(GL_W32, 1 << (32 - n_bits), P)


def f3_pow(a, e):
    r, b = ONE3, f3(a)
    while e:
        if e & 1:
            r = f3_mul(r, b)
        b = f3_mul(b, b)
        e >>= 1
    return r


def f3_scale(a, s):
    return tuple(v * s % P for v in a)


XI_LAZY = (P + 3, M64, P + 1)       # == (3, 2^32 - 2, 1): every word at or above p
XI_BASE_LAZY = (P + 5, P, 0)        # == (5, 0, 0): the base field, written with lazy words


def rand_xi(rng):
    """a canonical F_p^3 element with non-zero second and third components:
    x - xi is then non-zero for every base-field x"""
    return tuple(int(v) for v in rng.integers(1, P, size=3, dtype=np.uint64))


def lazy_ext(rng):
    """lazy words of an element with non-zero second and third components"""
    return (P + int(rng.integers(0, EPS)), M64, P + 1 + int(rng.integers(0, EPS - 1)))


# ------------------------------------------------------------------ LEv / LpEv, xDivXSub
def _x_over_x_minus(x, a):
    """x / (x - a), x in F_p, a in F_p^3 outside F_p"""
    di = f3_inv(((x - a[0]) % P, -a[1] % P, -a[2] % P))
    return f3_scale(di, x)


def ref_lagrange(xi, n_bits, rows):
    """(LEv rows, LpEv rows) in closed form: LEv[k] = ((1 - xi^N) / N) x_k / (x_k - xi),
    x_k = w_N^k; LpEv with w_N xi in place of xi ((w_N xi)^N = xi^N: the same scale)"""
    xi = f3(xi)
    n = 1 << n_bits
    w = gl_w(n_bits)
    wxi = f3_scale(xi, w)
    p = f3_pow(xi, n)
    scale = f3_scale(((1 - p[0]) % P, -p[1] % P, -p[2] % P), pow(n, -1, P))
    lev, lpev = [], []
    for k in rows:
        x = pow(w, k, P)
        lev.append(f3_mul(_x_over_x_minus(x, xi), scale))
        lpev.append(f3_mul(_x_over_x_minus(x, wxi), scale))
    return lev, lpev


def ref_xdivxsub(xi, n_bits, n_bits_ext, rows):
    """(xDivXSubXi rows, xDivXSubWXi rows): x_k / (x_k - xi) and x_k / (x_k - w_N xi), x_k = 7 w_NE^k"""
    xi = f3(xi)
    wxi = f3_scale(xi, gl_w(n_bits))
    we = gl_w(n_bits_ext)
    a, b = [], []
    for k in rows:
        x = 7 * pow(we, k, P) % P
        a.append(_x_over_x_minus(x, xi))
        b.append(_x_over_x_minus(x, wxi))
    return a, b


def row_blocks(n):
    """(row0, nrows) of a 2^k-row domain, n >= 512: one row at either end; a
    thread's chunk of 16 less one, exactly, plus one; half the domain, one row
    more (at n = 8192: 4096 rows fill one workgroup, 4097 double the thread
    stride T), the same ending exactly at n; the whole domain; nothing"""
    h = n // 2
    return [(0, 1), (n - 1, 1), (5, BI_CHUNK - 1), (16, BI_CHUNK), (3, BI_CHUNK + 1), (0, h), (100, h + 1),
            (h - 1, h + 1), (0, n), (n, 0)]


def xdiv_threads(nrows):
    """T of k_xdiv_rows: thread t owns rows t + j T, j < BI_CHUNK"""
    per = (nrows + BI_CHUNK - 1) // BI_CHUNK
    return (per + XDIV_THREADS - 1) // XDIV_THREADS * XDIV_THREADS


LAG_NBITS = 13
LAG_BLOCKS = [(0, 1), (8191, 1), (5, 15), (16, 16), (3, 17), (0, 4096), (100, 4097), (4095, 4097), (0, 8192),
              (8192, 0)]
LAG_SMALL_NBITS = [0, 1, 4]
LAG_BIG_NBITS = [24, 28]            # twiddle exponents in the high table's upper entries; closed form only


def big_blocks(n_bits):
    n = 1 << n_bits
    return [(0, 33), (n - 100, 100), (n // 2 - 7, 50)]


XDIV_ROWS_BITS = [(8, 9), (11, 13), (10, 10)]   # (n_bits, n_bits_ext)
XDIV_WHOLE_BITS = [(0, 1), (3, 4), (11, 13)]


def tw_index(row, logn):
    """(low, high) twiddle-table indices of row `row` of a 2^logn domain"""
    ex = (row & ((1 << logn) - 1)) << (TW_MAX_LOG - logn)
    return ex & ((1 << TW_LEVEL_BITS) - 1), ex >> TW_LEVEL_BITS


# ------------------------------------------------------------------ evmap
EV_N = [1, 255, 256, 257, 511, 513, 61439, 61440, 61441]
EV_EB = [0, 2]
EV_LIST_N = 513                     # every entry list runs here: two iterations of 512 rows, the second ragged
EV_SPLIT = (61441, 30001)           # the prover's row blocks [0, k) and [k, n); k is no multiple of 256

# entries: (polynomial, dim, prime); a polynomial is dim columns one leading dimension apart
EV_SHAPE_ENTRIES = [(0, 1, 0), (1, 1, 0), (2, 3, 0), (3, 3, 1), (4, 1, 1), (5, 1, 1)]


def _mixed45():
    rng = np.random.default_rng(45)
    return [(e, int(rng.choice([1, 3])), int(rng.integers(0, 2))) for e in range(45)]


EV_LISTS = {
    "one_dim1": [(0, 1, 0)],
    "four_same_prime": [(e, 1, 1) for e in range(4)],
    "five_same_prime": [(e, 1, 0) for e in range(5)],
    "dim3_straddles": [(0, 1, 0), (1, 1, 0), (2, 3, 0), (3, 1, 0)],
    "all_prime": [(0, 3, 1), (1, 1, 1), (2, 3, 1)],
    "one_column_twice": [(0, 1, 0), (0, 1, 1), (1, 3, 1), (1, 3, 0)],
    "mixed45": _mixed45(),
    "empty": [],
    "shape": EV_SHAPE_ENTRIES,
}


def ev_groups(entries):
    """zkgpu_evmap_dev's grouping: sub-entries (entry, component) in entry
    order, stably sorted by prime, cut into groups of at most EV_GW with one
    prime each -> [(prime, [(entry, component)])]"""
    subs = [(1 if prime else 0, e, j) for e, (_, dim, prime) in enumerate(entries) for j in range(dim)]
    subs.sort(key=lambda s: s[0])
    groups = []
    for prime, e, j in subs:
        if not groups or groups[-1][0] != prime or len(groups[-1][1]) == EV_GW:
            groups.append((prime, []))
        groups[-1][1].append((e, j))
    return groups


def ev_l_ld(n):
    return n + 7


def ev_col_ld(n, eb, e):
    return (n << eb) + 3 + e


def ev_span(n, eb):
    """rows of a column that n rows at stride 2^eb reach"""
    return ((n - 1) << eb) + 1 if n else 0


class EvCase:
    """lev, lpev: (3, n) lazy words; polys: {polynomial: (dim, n) lazy words}
    (the values at the rows k << eb); ld[polynomial]: the leading dimension of
    its columns, that of the first entry naming it"""

    def __init__(self, n, eb, entries, seed=0):
        rng = np.random.default_rng([n, eb, len(entries), seed])
        self.n, self.eb, self.entries = n, eb, list(entries)
        self.lev = lazy(canonical(rng, (3, n)))
        self.lpev = lazy(canonical(rng, (3, n)))
        self.polys, self.ld = {}, {}
        for e, (poly, dim, _) in enumerate(self.entries):
            if poly not in self.polys:
                self.polys[poly] = lazy(canonical(rng, (dim, n)))
                self.ld[poly] = ev_col_ld(n, eb, e)
            assert self.polys[poly].shape[0] == dim
        self.dims = np.array([d for _, d, _ in self.entries], np.uint32)
        self.primes = np.array([p for _, _, p in self.entries], np.uint32)

    def poly_image(self, poly, fill, guard):
        """the device words of a polynomial: dim columns of ld words, the
        values at the rows k << eb and `fill` in every other word"""
        v, ld = self.polys[poly], self.ld[poly]
        img = np.full(v.shape[0] * ld + guard, fill, dtype=np.uint64)
        for j in range(v.shape[0]):
            img[j * ld:j * ld + ev_span(self.n, self.eb):1 << self.eb] = v[j]
        return img


def ref_evmap(case, r0=0, r1=None):
    """evals[e] = sum_{r0 <= k < r1} L(k) pol_e[k] in Python integers -> (n_ev, 3) uint64"""
    r1 = case.n if r1 is None else r1
    L = {0: rows3(case.lev[:, r0:r1]), 1: rows3(case.lpev[:, r0:r1])}
    out = np.zeros((len(case.entries), 3), np.uint64)
    for e, (poly, dim, prime) in enumerate(case.entries):
        v = case.polys[poly][:, r0:r1]
        acc = [0, 0, 0]
        if dim == 1:
            for l, a in zip(L[1 if prime else 0], (int(x) % P for x in v[0])):
                acc = [acc[0] + l[0] * a, acc[1] + l[1] * a, acc[2] + l[2] * a]
        else:
            for l, p in zip(L[1 if prime else 0], rows3(v)):
                t = f3_mul(l, p)
                acc = [acc[0] + t[0], acc[1] + t[1], acc[2] + t[2]]
        out[e] = [a % P for a in acc]
    return out


def oracle_evmap(oc, case, r0=0, r1=None):
    """the same through the oracle's Starks::evmap on the inputs reduced mod p
    (row-major, the values only: stride dim, extend_bits 0)"""
    r1 = case.n if r1 is None else r1
    n, n_ev = r1 - r0, len(case.entries)
    out = np.zeros((n_ev, 3), np.uint64)
    if not n_ev:
        return out
    pn = np.uint64(P)
    rows = {poly: np.ascontiguousarray((v[:, r0:r1] % pn).T) for poly, v in case.polys.items()}
    ptrs = (ctypes.c_void_p * n_ev)(*[rows[poly].ctypes.data for poly, _, _ in case.entries])
    strides = np.array([d for _, d, _ in case.entries], np.uint64)
    lev = np.ascontiguousarray((case.lev[:, r0:r1] % pn).T)
    lpev = np.ascontiguousarray((case.lpev[:, r0:r1] % pn).T)
    oc.lib().oc_evmap(oc._p(out), ctypes.cast(ptrs, ctypes.c_void_p), ctypes.c_void_p(strides.ctypes.data),
                      ctypes.c_void_p(case.dims.ctypes.data), ctypes.c_void_p(case.primes.ctypes.data), n_ev,
                      oc._p(lev), oc._p(lpev), n, 0)
    return out


def add_evals(a, b):
    """(n_ev, 3) + (n_ev, 3) mod p"""
    s = [[(int(x) + int(y)) % P for x, y in zip(ra, rb)] for ra, rb in zip(a, b)]
    return np.array(s, dtype=np.uint64).reshape(-1, 3)


# ------------------------------------------------------------------ FRI
FOLD_WHOLE = [(0, 0), (1, 0), (3, 1), (3, 0), (5, 1), (5, 0), (13, 8), (14, 9), (9, 9)]  # (pol_bits, out_bits)
FOLD_ROWS_BITS = [16, 24, 28]
FOLD_ROWS_REDUCTION = [2, 5]
FOLD_ROWS_NG = [1, 257]             # one group; two workgroups, the second with one thread at work


def fold_seam_g0(pol_bits, out_bits, ng):
    """g0 of a block whose twiddle exponents (g0 + j) << (28 - pol_bits) cross
    a multiple of 2^14, where the low table wraps and the high index steps
    (ng = 1: the group on the multiple itself)"""
    m = 1 << max(0, pol_bits - TW_LEVEL_BITS)   # groups per step of the high index
    seam = (3 << out_bits) // 4 // m * m
    return seam - ng // 2


def fold_rows_g0(pol_bits, out_bits, ng):
    return [0, (1 << out_bits) - ng, fold_seam_g0(pol_bits, out_bits, ng)]


def fold_tw_index(g, pol_bits):
    e = g << (TW_MAX_LOG - pol_bits)
    return e & ((1 << TW_LEVEL_BITS) - 1), e >> TW_LEVEL_BITS


def fold_shift_inv(rng):
    """a word at or above p (the kernel's shift_inv is any word)"""
    return P + int(rng.integers(2, EPS))


FRI_TRANSPOSE = [(1, 0), (8, 0), (8, 3), (4096, 1), (4096, 11), (96, 5), (257 * 4, 2)]  # (degree, transpose_bits)

# ------------------------------------------------------------------ openings
OPEN_NROWS = [1, 2, 4, 1024]        # no level (empty siblings), one, two, ten
OPEN_NCOLS = [0, 1, 4, 63, 64, 65, 130]   # the 64 threads' column loop: none, short, exact, one more, three passes
OPEN_NQ = [1, 300]


def open_indices(nrows, nq, rng):
    """unsorted, with repeats, holding row 0 and row nrows - 1 (nq = 1: the last row)"""
    if nq == 1:
        return np.array([nrows - 1], np.uint64)
    idx = rng.integers(0, nrows, nq, dtype=np.uint64)
    idx[1], idx[nq // 2], idx[nq - 1], idx[0] = 0, nrows - 1, idx[2], nrows - 1
    return idx
