"""The row-block model of the expression evaluator (zkgpu_zxp_eval_block_dev).

A row-sharded prover cuts a 2^log_domain-row domain into blocks of 2^log_rows
rows; a block's owner holds its rows plus `halo` rows of the next block (the
domain's first rows after the last block) and calls the evaluator on that
local image: shifted reads run into the halo and do not wrap, a store at row
shift s lands on local row i + s, x_i = x_start w^i with w of the WHOLE
domain, zhInv is indexed by the local row and xdiv / xdivw arrive advanced to
the block's first row.  This module says, in numpy, what such a call must
leave behind, given the whole-domain evaluation (the oracle's oc_zxp_eval or
oc_parser_eval):

split      whole-domain sections -> per block column-major local images with
           poisoned pad rows and guard words
expected   the images after a block call: the stored regions from the whole
           domain's result, every other word as loaded
recompose  the whole-domain stored columns from all blocks' stored regions,
           every cell from exactly one block
assert_block / assert_recomposed   the comparisons both the CPU stand-in
           (tests/test_block_cases.py) and the device (tests/test_gpu_zxp_eval_block.py) face

and builds three small programs (stage, quotient, fri) that use every operand
kind and every block-mode rule, with inputs that are half non-canonical.
"""
import ctypes

import numpy as np

from zkgpu.synthetic import (ADD, COL, COL3, COPY, MUL, PUB, SEC_CM1_2NS, SEC_CM1_N, SEC_CM2_N, SEC_CM3_2NS, SEC_CM3_N,
                             SEC_CONST_2NS, SEC_CONST_N, SEC_F_2NS, SEC_Q_2NS, SEC_TMP_N, SUB, X, XDIV, XDIVW, ZI,
                             Program)

P = 0xFFFFFFFF00000001
POISON = 0xA5A5A5A5A5A5A5A5
GUARD = 5  # words after a section's last column
W32 = 7277203076849721926  # of order 2^32
EDGE = (0, 1, P - 1, P, P + 1, (1 << 64) - 1)


def gl_w(n):
    w = W32
    for _ in range(n, 32):
        w = w * w % P
    return w


def _shift(c):
    c = int(c)
    return c - (1 << 32) if c >= 1 << 31 else c


# ---------------------------------------------------------------- geometry
class Geom:
    """One way of cutting a domain: 2^(log_domain - log_rows) blocks whose local
    columns are ld = 2^log_rows + halo + pad rows long."""

    def __init__(self, log_domain, log_rows, halo, pad, guard=GUARD):
        assert 0 <= log_rows <= log_domain and halo >= 0 and pad >= 0
        self.log_domain, self.log_rows, self.halo, self.pad, self.guard = log_domain, log_rows, halo, pad, guard
        self.N, self.rows = 1 << log_domain, 1 << log_rows
        self.ld = self.rows + halo + pad
        self.nblocks = 1 << (log_domain - log_rows)

    def row0(self, b):
        return b << self.log_rows

    def words(self, width):
        return width * self.ld + self.guard

    def columns(self, img, width):
        """(width, ld) view of a local image's columns"""
        return img[:width * self.ld].reshape(width, self.ld)


def split(S, log_domain, log_rows, halo, pad, guard=GUARD):
    """S: {section: (N, width) whole-domain array} -> per block {section: local
    image}: a flat array of `width` columns of ld rows, then `guard` words.
    Local row r < 2^log_rows + halo holds whole row (row0 + r) mod N; the pad
    rows and the guard words hold POISON."""
    g = Geom(log_domain, log_rows, halo, pad, guard)
    out = []
    for b in range(g.nblocks):
        idx = (g.row0(b) + np.arange(g.rows + halo)) % g.N
        blk = {}
        for sec, A in S.items():
            assert A.shape[0] == g.N
            img = np.full(g.words(A.shape[1]), POISON, np.uint64)
            g.columns(img, A.shape[1])[:, :g.rows + halo] = A[idx].T
            blk[sec] = img
        out.append(blk)
    return out


def x_start(log_domain, row0, ext):
    """x of a block's first row: w^row0, on the extended domain's coset 7 w^row0"""
    return (7 if ext else 1) * pow(gl_w(log_domain), row0, P) % P


def xdiv_words(xdiv, row0):
    """the block's xdiv / xdivw: the whole (N, 3) array from word 3 row0 on"""
    return xdiv.reshape(-1)[3 * row0:]


def stores_of(prog):
    """{(section, column): row shift} of a program's destination operands"""
    ins, opn = prog.arrays()
    out = {}
    for _op, dst, _a, _b in ins.tolist():
        kind, sec, col, c = opn[dst].tolist()
        if kind in (COL, COL3):
            for k in range(3 if kind == COL3 else 1):
                assert out.setdefault((sec, col + k), _shift(c)) == _shift(c), "a column stored at two shifts"
    return out


def max_shift(prog):
    """the halo a program needs: its largest row shift, read or stored"""
    _ins, opn = prog.arrays()
    sh = [_shift(c) for kind, _a, _b, c in opn.tolist() if kind in (COL, COL3)]
    assert min(sh) >= 0
    return max(sh)


def expected(S_before, S_after_whole, stores, g):
    """The local images a block call must leave, per block: a column stored at
    shift s has local rows [s, 2^log_rows + s) equal to the whole domain's
    result at rows (row0 + r) mod N; its rows [0, s), its rows from
    2^log_rows + s on, and every other word -- unstored columns, halo, pad,
    guard -- are as loaded."""
    out = split(S_before, g.log_domain, g.log_rows, g.halo, g.pad, g.guard)
    for b, blk in enumerate(out):
        for (sec, col), s in stores.items():
            assert 0 <= s <= g.halo
            idx = (g.row0(b) + np.arange(s, g.rows + s)) % g.N
            g.columns(blk[sec], S_before[sec].shape[1])[col, s:g.rows + s] = S_after_whole[sec][idx, col]
    return out


def recompose(blocks, stores, widths, g):
    """{(section, column): whole-domain column} from every block's stored
    region; each whole-domain cell of a stored column comes from exactly one
    block (asserted)."""
    out = {}
    for (sec, col), s in stores.items():
        whole = np.zeros(g.N, np.uint64)
        seen = np.zeros(g.N, np.int64)
        for b, blk in enumerate(blocks):
            idx = (g.row0(b) + np.arange(s, g.rows + s)) % g.N
            whole[idx] = g.columns(blk[sec], widths[sec])[col, s:g.rows + s]
            np.add.at(seen, idx, 1)
        assert (seen == 1).all(), "section %d column %d: row %d comes from %d blocks" % (
            sec, col, int(np.argmax(seen != 1)), int(seen[np.argmax(seen != 1)]))
        out[(sec, col)] = whole
    return out


def assert_block(got, want, widths, g, b):
    """a block's images word for word, pad rows and guard words included"""
    for sec in sorted(want):
        if np.array_equal(got[sec], want[sec]):
            continue
        k = int(np.argmax(got[sec] != want[sec]))
        n = int((got[sec] != want[sec]).sum())
        w = widths[sec]
        where = "guard word %d" % (k - w * g.ld) if k >= w * g.ld else "column %d local row %d (global %d)" % (
            k // g.ld, k % g.ld, (g.row0(b) + k % g.ld) % g.N)
        raise AssertionError("block %d (row0 %d) section %d: %d words differ, first at %s: %#x, expected %#x" % (
            b, g.row0(b), sec, n, where, int(got[sec][k]), int(want[sec][k])))


def assert_recomposed(blocks, stores, S_after_whole, widths, g):
    """all blocks' stored regions put together == the whole domain's result"""
    for (sec, col), whole in sorted(recompose(blocks, stores, widths, g).items()):
        ref = S_after_whole[sec][:, col]
        bad = np.flatnonzero(whole != ref)
        assert bad.size == 0, "section %d column %d: %d rows differ from the whole domain, first %d" % (
            sec, col, bad.size, int(bad[0]))


# ---------------------------------------------------------------- programs
N_PUB, N_EV = 4, 12


class Case:
    def __init__(self, name, prog, widths, log_domain, ext, eb):
        self.name, self.prog, self.widths = name, prog, widths
        self.log_domain, self.ext, self.eb = log_domain, ext, eb
        self.stores = stores_of(prog)
        self.halo = max_shift(prog)


def stage():
    """n domain, 2^10 rows.  Reads COL / COL3 at shift 0 and +1, X, CHAL, PUB,
    LIT; a product of two row-varying base values and one of two F_p^3 columns;
    a 12-term sum (a DOT3 once compiled); stores a COL and a COL3 at shift 0,
    a COL at shift +1 and a COL3 at shift +2.  No stored column is read."""
    p = Program(0)

    def a(c, s=0):
        return p.col(SEC_CM1_N, c, s)

    t, u, e, g = p.tmp1(), p.tmp1(), p.tmp3(), p.tmp3()
    p.op(MUL, t, a(0), a(1, 1))
    p.op(MUL, u, p.o(X), p.col(SEC_CONST_N, 0, 1))
    p.op(ADD, t, t, u)
    p.op(ADD, t, t, p.o(PUB, 1))
    p.op(COPY, p.col(SEC_TMP_N, 0), t)
    p.op(MUL, e, p.chal(0), a(2))
    for k in range(1, 12):
        p.op(MUL, g, p.chal(k % 8), a(2 + k, k % 2))
        p.op(ADD, e, e, g)
    p.op(ADD, e, e, p.col3(SEC_CM2_N, 0, 1))
    p.op(MUL, g, p.col3(SEC_CM2_N, 3), p.col3(SEC_CM2_N, 0))
    p.op(ADD, e, e, g)
    p.op(COPY, p.col3(SEC_CM3_N, 0), e)
    p.op(MUL, u, a(3, 1), p.lit(0x1234567890ABCDEF))
    p.op(SUB, u, u, t)
    p.op(ADD, u, u, p.col(SEC_CONST_N, 1))
    p.op(COPY, p.col(SEC_TMP_N, 1, 1), u)
    p.op(MUL, g, e, p.o(X))
    p.op(SUB, g, g, p.col3(SEC_CM2_N, 3, 1))
    p.op(ADD, g, g, p.lit(7))
    p.op(COPY, p.col3(SEC_CM3_N, 3, 2), g)
    # (tmpExp column 2 and cm3 column 6 are never stored: they must stay as loaded)
    return Case("stage", p, {SEC_CM1_N: 14, SEC_CM2_N: 6, SEC_CONST_N: 2, SEC_TMP_N: 3, SEC_CM3_N: 7}, 10, False, 0)


def quotient(eb):
    """extended domain of 2^(10 + eb) rows: three constraints combined with
    challenge 4, "next row" reads at shift 2^eb, then x X, then x ZI stored to
    COL3(SEC_Q_2NS, 0)."""
    p = Program(1)
    nxt = 1 << eb

    def a(c, s=0):
        return p.col(SEC_CM1_2NS, c, s)

    acc, r, s, t = p.tmp3(), p.tmp3(), p.tmp3(), p.tmp1()
    alpha, gamma = p.chal(4), p.chal(2)
    p.op(MUL, t, a(0), a(1))
    p.op(MUL, t, t, p.col(SEC_CONST_2NS, 0))
    p.op(ADD, t, t, a(0))
    p.op(SUB, t, a(2), t)
    p.op(COPY, acc, t)
    p.op(ADD, r, p.col3(SEC_CM3_2NS, 0, nxt), gamma)
    p.op(MUL, r, r, p.col3(SEC_CM3_2NS, 3, nxt))
    p.op(ADD, s, p.col3(SEC_CM3_2NS, 0), gamma)
    p.op(MUL, s, s, p.col3(SEC_CM3_2NS, 3))
    p.op(SUB, r, r, s)
    p.op(MUL, acc, acc, alpha)
    p.op(ADD, acc, acc, r)
    p.op(SUB, t, a(3, nxt), a(3))
    p.op(SUB, t, t, p.o(PUB, 0))
    p.op(MUL, t, t, p.col(SEC_CONST_2NS, 1, nxt))
    p.op(MUL, acc, acc, alpha)
    p.op(ADD, acc, acc, t)
    p.op(MUL, s, p.chal(0), a(4))
    p.op(MUL, r, p.chal(1), a(5, nxt))
    p.op(ADD, s, s, r)
    p.op(ADD, s, s, p.lit(P - 3))
    p.op(MUL, acc, acc, alpha)
    p.op(ADD, acc, acc, s)
    p.op(MUL, acc, acc, p.o(X))
    p.op(MUL, p.col3(SEC_Q_2NS, 0), acc, p.o(ZI))
    return Case("quotient%d" % eb, p, {SEC_CM1_2NS: 6, SEC_CM3_2NS: 6, SEC_CONST_2NS: 2, SEC_Q_2NS: 4}, 10 + eb, True,
                eb)


def fri():
    """extended domain, 2^12 rows: a Horner chain with challenge 5 over base
    and F_p^3 columns, then for XDIV and XDIVW a Horner chain with challenge 6
    over (column - EVAL) times the operand; stored to COL3(SEC_F_2NS, 0)."""
    p = Program(1)
    v1, v2 = p.chal(5), p.chal(6)
    cols = [p.col(SEC_CM1_2NS, c) for c in range(5)] + [p.col3(SEC_CM3_2NS, 0), p.col3(SEC_CM3_2NS, 3)]
    acc = p.tmp3()
    p.op(MUL, acc, cols[0], v1)
    for c in cols[1:]:
        p.op(MUL, acc, acc, v1)
        p.op(ADD, acc, acc, c)
    e = 0
    for kind, members in ((XDIV, cols), (XDIVW, cols[1::2])):
        g, d = p.tmp3(), p.tmp3()
        for k, c in enumerate(members):
            p.op(SUB, d, c, p.ev(e))
            e += 1
            if k == 0:
                p.op(COPY, g, d)
            else:
                p.op(MUL, g, g, v2)
                p.op(ADD, g, g, d)
        p.op(MUL, g, g, p.o(kind))
        p.op(ADD, acc, acc, g)
    assert e <= N_EV
    p.op(COPY, p.col3(SEC_F_2NS, 0), acc)
    return Case("fri", p, {SEC_CM1_2NS: 5, SEC_CM3_2NS: 6, SEC_F_2NS: 4}, 12, True, 1)


CASES = {"stage": stage, "quotient1": lambda: quotient(1), "quotient2": lambda: quotient(2), "fri": fri}
# log_rows: W = 1, a quarter of the domain, one interpreter workgroup, fewer rows than a wave
LOG_ROWS = {name: (ld, ld - 2, 6, 4) for name, ld in (("stage", 10), ("quotient1", 11), ("quotient2", 12), ("fri", 12))}
PADS = (0, 3)


# ---------------------------------------------------------------- inputs
def lazy_words(rng, shape):
    """half random canonical, half from EDGE (non-canonical words included)"""
    a = rng.integers(0, P, size=shape, dtype=np.uint64)
    edge = np.array(EDGE, np.uint64)[rng.integers(0, len(EDGE), size=shape)]
    return np.where(rng.integers(0, 2, size=shape).astype(bool), a, edge)


class Inputs:
    """S: the sections as loaded (lazy words); S_canon: the same mod p, what
    the oracle is given; canonical scalars; random xdiv / xdivw arrays."""

    def __init__(self, case, seed):
        rng = np.random.default_rng(seed)
        N = 1 << case.log_domain
        self.N = N
        self.S = {sec: lazy_words(rng, (N, w)) for sec, w in sorted(case.widths.items())}
        self.S_canon = {sec: a % np.uint64(P) for sec, a in self.S.items()}
        self.chal = rng.integers(0, P, size=(8, 3), dtype=np.uint64)
        self.pub = rng.integers(0, P, size=N_PUB, dtype=np.uint64)
        self.evals = rng.integers(0, P, size=(N_EV, 3), dtype=np.uint64)
        self.xdiv = rng.integers(0, P, size=(N, 3), dtype=np.uint64)
        self.xdivw = rng.integers(0, P, size=(N, 3), dtype=np.uint64)
        w = gl_w(case.log_domain)
        x = [7 if case.ext else 1]
        for _ in range(N - 1):
            x.append(x[-1] * w % P)
        self.x = np.array(x, np.uint64)
        # zhInv[j] = 1 / (7^n w_{2^eb}^j - 1), n = N / 2^eb rows of the trace domain
        n = N >> case.eb
        we = gl_w(case.eb) if case.eb else 1
        self.zh = np.array([pow((pow(7, n, P) * pow(we, j, P) - 1) % P, P - 2, P) for j in range(1 << case.eb)],
                           np.uint64) if case.ext else np.ones(1, np.uint64)


def oracle_whole(oracle, case, inp):
    """The sections after the oracle's oc_zxp_eval over the whole domain
    (oracle/stark.c; shifted reads and stores wrap at N), from S_canon."""
    S = {k: np.ascontiguousarray(a.copy()) for k, a in inp.S_canon.items()}
    secs = (ctypes.c_void_p * 12)()
    strides = np.zeros(12, np.uint64)
    for k, a in S.items():
        secs[k] = a.ctypes.data
        strides[k] = a.shape[1]
    ins, opn = case.prog.arrays()
    ins = np.ascontiguousarray(ins, np.uint32)
    opn = np.ascontiguousarray(opn, np.uint32)
    p = oracle._p
    oracle.lib().oc_zxp_eval(ctypes.c_void_p(ins.ctypes.data), ins.shape[0], ctypes.c_void_p(opn.ctypes.data),
                             max(case.prog.n_tmp1, 1), max(case.prog.n_tmp3, 1), ctypes.cast(secs, ctypes.c_void_p),
                             ctypes.c_void_p(strides.ctypes.data), inp.N, p(inp.chal), p(inp.pub), p(inp.evals),
                             p(inp.x), p(inp.xdiv), p(inp.xdivw), p(inp.zh), inp.zh.size)
    return S
