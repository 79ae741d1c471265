"""Worst-case operands and long forms for the dot-product layer (Dot3).

Every linear combination of the expression programs and of the evaluation map
runs through Dot3 (csrc/gl_device.hpp): three u64 accumulators fed by
carry-free 32x32 multiply-adds, reduced once.  Nothing but a term count keeps
them below 2^64, and five places keep such a count (DESIGN.md "Dot3 term
counts").  Uniformly random operands leave a 250-term accumulator near 2^61,
a quarter of the worst case, so a count wrong by a factor of two would pass
every random-input test.  This module restates Dot3 in Python integers
(`limbs6`, `Dot3`, `accumulators`), gives operands that drive all three
accumulators to 0.9 of their per-term maximum at once (`A_MAX`, `C_JOINT`),
builds programs whose forms are long enough to reach each count
(`wide_sum`, `chains`, `combine_store`, `temp_terms`) and lays out sections
with whole blocks of worst-case rows (`Inputs`).
tests/test_dot_cases.py checks all of it on the CPU; tests/test_gpu_dot_cases.py
runs the programs and the evaluation map on the GPU.
"""
import ctypes

import numpy as np

from zkgpu.synthetic import ADD, COL, COL3, COPY, MUL, PUB, SEC_CM1_N, SEC_TMP_N, TMP1, TMP3, Program

P = 0xFFFFFFFF00000001
M64 = (1 << 64) - 1
M32 = 0xFFFFFFFF
ZXP_DOT1, ZXP_DOT3 = 4, 5  # include/zkgpu_zxp.h
ZXP_TERM_ONE = 0xFFFFFFFF

# per-term maxima of the three accumulators (both halves of the source at
# 2^32 - 1, both limbs of the accumulator's weight all ones)
LIMB_MAX = ((1 << 22) - 1, (1 << 21) - 1, (1 << 21) - 1)
TERM_MAX = tuple(2 * M32 * m for m in LIMB_MAX)
DOT_CAP = 250  # DOT_HARD_CAP (csrc/zxp_compile.cpp): terms per DOT, the constant included

# the canonical word with both halves at or next to 2^32 - 1
A_MAX = 0xFFFFFFFEFFFFFFFF


# ---------------------------------------------------------------- Dot3 model
def limbs6(c):
    """Dot3 limbs of a coefficient: 22/21/21 bits of c and of c 2^32 mod p
    (api.hip zxp_limbs6 for canonical c; Dot3::limbs takes any u64)."""
    cs = (c << 32) % P
    return (c & 0x3FFFFF, (c >> 22) & 0x1FFFFF, c >> 43, cs & 0x3FFFFF, (cs >> 22) & 0x1FFFFF, cs >> 43)


def fin_words(a0, a1, a2):
    """Dot3::fin on three u64 words: the 128-bit sum (l2, h) of the weighted
    accumulators as the device forms it, reduced mod p."""
    assert max(a0, a1, a2) <= M64
    l1 = a0 + ((a1 << 22) & M64)
    c1, l1 = l1 >> 64, l1 & M64
    l2 = l1 + ((a2 << 43) & M64)
    c2, l2 = l2 >> 64, l2 & M64
    h = (a1 >> 42) + (a2 >> 21) + c1 + c2
    return (l2 + (h << 64)) % P


class Dot3:
    """gl_device.hpp Dot3 with unbounded accumulators: `acc` is what an ideal
    machine holds, `fin` what the 64-bit registers give (equal below 2^64)."""

    def __init__(self, cst=0):
        # Dot3(const uint32_t *k): the constant's 22/21/21-bit limbs
        self.acc = [cst & 0x3FFFFF, (cst >> 22) & 0x1FFFFF, cst >> 43]

    def term(self, a, l6):
        a0, a1 = a & M32, a >> 32
        for j in range(3):
            self.acc[j] += a0 * l6[j] + a1 * l6[3 + j]

    def lane(self, a):
        self.acc[0] += a & M32
        self.acc[1] += (a >> 32) << 10

    def fin(self):
        return fin_words(*[x & M64 for x in self.acc])

    def exact(self):
        return (self.acc[0] + (self.acc[1] << 22) + (self.acc[2] << 43)) % P


def dot_instrs(comp):
    """(instruction index, first term, term count, components) of every DOT."""
    return [(k, int(a), int(b), 3 if op == ZXP_DOT3 else 1)
            for k, (op, _d, a, b) in enumerate(comp["instr"]) if op in (ZXP_DOT1, ZXP_DOT3)]


def accumulators(comp, k, source_values):
    """The Dot3 accumulators of DOT instruction k of a compiled program
    (zkgpu.zxp_compile): per result component, ([A0, A1, A2], reduced value).
    source_values(operand row (kind, a, b, c), component) -> u64 source word."""
    op, _dst, first, count = (int(x) for x in comp["instr"][k])
    assert op in (ZXP_DOT1, ZXP_DOT3)
    terms = comp["term"][first:first + count]
    out = []
    for j in range(3 if op == ZXP_DOT3 else 1):
        cst = sum(int(t["coef"][j]) for t in terms if int(t["src"]) == ZXP_TERM_ONE) % P
        d = Dot3(cst)
        for t in terms:
            if int(t["src"]) == ZXP_TERM_ONE:
                continue
            a = source_values(tuple(int(x) for x in comp["opnd"][int(t["src"])]), int(t["comp"]))
            d.term(a, limbs6(int(t["coef"][j]) % P))
        out.append((list(d.acc), d.fin()))
    return out


def _mul2_32(c):
    """c 2^32 mod p on a uint64 array of canonical values."""
    hi, lo = c >> np.uint64(32), c & np.uint64(M32)
    t1 = hi * np.uint64(M32)
    s = t1 + (lo << np.uint64(32))
    s = s + (s < t1).astype(np.uint64) * np.uint64(M32)  # 2^64 = 2^32 - 1
    return np.where(s >= np.uint64(P), s - np.uint64(P), s)


def limb_sums(c):
    """(l0 + l3, l1 + l4, l2 + l5) of a uint64 array of canonical coefficients."""
    cs = _mul2_32(c)
    m22, m21 = np.uint64(0x3FFFFF), np.uint64(0x1FFFFF)
    return ((c & m22) + (cs & m22), ((c >> np.uint64(22)) & m21) + ((cs >> np.uint64(22)) & m21),
            (c >> np.uint64(43)) + (cs >> np.uint64(43)))


def static_headroom(comp):
    """Largest accumulator any DOT of the program reaches with every source
    word at 2^64 - 1 and the program's own coefficient limbs -> (max, terms of
    that DOT)."""
    best = (0, 0)
    term = comp["term"]
    if not len(term):
        return best
    one = term["src"] == ZXP_TERM_ONE
    for j in range(3):
        c = term["coef"][:, j] % np.uint64(P)
        sums = limb_sums(c)
        for w in range(3):
            # a constant enters through its own limbs only (Dot3's constructor)
            cl = [c & np.uint64(0x3FFFFF), (c >> np.uint64(22)) & np.uint64(0x1FFFFF), c >> np.uint64(43)][w]
            per = np.where(one, cl, sums[w] * np.uint64(M32)).astype(object)
            tot = np.concatenate([[0], np.cumsum(per)])
            for _k, a, b, dim in dot_instrs(comp):
                if j < dim:
                    best = max(best, (int(tot[a + b] - tot[a]), b))
    return best


# ---------------------------------------------------------------- worst coefficients
def ratios(c):
    """Share of the per-term maximum coefficient c reaches in A0, A1, A2."""
    l = limbs6(c)
    return tuple((l[j] + l[3 + j]) / (2 * LIMB_MAX[j]) for j in range(3))


SEARCH_SEED, SEARCH_SAMPLES = 0xD073, 1 << 24


def search_pool(seed=SEARCH_SEED, samples=SEARCH_SAMPLES):
    """Seeded random search: the coefficient maximising each limb-pair sum and
    the one maximising the smallest of the three ratios."""
    rng = np.random.default_rng(seed)
    best = [(-1.0, 0)] * 4
    for _ in range(samples >> 18):
        c = rng.integers(0, P, size=1 << 18, dtype=np.uint64)
        r = [s.astype(np.float64) / (2 * m) for s, m in zip(limb_sums(c), LIMB_MAX)]
        r.append(np.minimum(np.minimum(r[0], r[1]), r[2]))
        for j in range(4):
            i = int(np.argmax(r[j]))
            best[j] = max(best[j], (float(r[j][i]), int(c[i])))
    return tuple(c for _r, c in best)


# search_pool() at the seed and sample count above (test_dot_cases.py re-runs it)
C_TOP0 = 0xC00003B0767FFB94  # l0 + l3 at 0.9998 of its maximum
C_TOP1 = 0xB58C47FFC49E7800  # l1 + l4 at 0.9998
C_TOP2 = 0xFFF41CF5000779D8  # l2 + l5 at 0.9999
C_JOINT = 0xFD427F4BF37C30A0  # all three at 0.95 or more
POOL = (C_JOINT, C_JOINT, C_JOINT, C_JOINT, C_JOINT, C_TOP0, C_JOINT, C_JOINT, C_JOINT, C_JOINT, C_JOINT, C_TOP1,
        C_JOINT, C_JOINT, C_JOINT, C_JOINT, C_JOINT, C_TOP2)


def pool_values(rng, shape):
    """Coefficients drawn from POOL (mostly the joint maximiser)."""
    return np.array(POOL, np.uint64)[rng.integers(0, len(POOL), size=shape)]


# ---------------------------------------------------------------- programs
N_PUB = 8
LOG_DOM = 10
SEC_IN, SEC_OUT = SEC_CM1_N, SEC_TMP_N


class Case:
    """A program with what it needs to run: section widths, eval count."""

    def __init__(self, name, prog, n_in, n_out, n_ev):
        self.name, self.prog, self.n_ev = name, prog, max(n_ev, 1)
        self.widths = {SEC_IN: n_in, SEC_OUT: n_out}


def _shift(k):
    return 1 if k % 3 == 1 else 0  # a third of the columns at the next row: the wrap mask is in play


def wide_sum(K, dim=3):
    """acc = sum_k coef(k) col(k) as MUL/ADD pairs, stored to a COL3 (dim 3:
    coef = ev(k)) or a COL (dim 1: coef = pub / lit, the literals from POOL)."""
    p = Program(0)
    acc, t = (p.tmp3(), p.tmp3()) if dim == 3 else (p.tmp1(), p.tmp1())
    for k in range(K):
        coef = p.ev(k) if dim == 3 else (p.o(PUB, k % N_PUB) if k % 2 else p.lit(POOL[k % len(POOL)] + k))
        p.op(MUL, acc if k == 0 else t, coef, p.col(SEC_IN, k, _shift(k)))
        if k:
            p.op(ADD, acc, acc, t)
    p.op(COPY, p.col3(SEC_OUT, 0) if dim == 3 else p.col(SEC_OUT, 0), acc)
    return Case("wide_sum(%d,%d)" % (K, dim), p, K, 3, K if dim == 3 else 0)


def chain_members(k, n_chains=3):
    """Chains column k sits in: at least two, every fourth column in all."""
    m = k % (n_chains + 1)
    return [g for g in range(n_chains) if m == n_chains or g != (n_chains - 1 - m)]


def chains(K, n_chains=3):
    """FRI-shaped: chain g is acc_g = acc_g chal(g) + ev(.) col(k) over the
    columns with g in chain_members(k); the accumulators are stored at the
    end.  With chal(g) = 1 the coefficient of col(k) is exactly its eval."""
    p = Program(0)
    t = p.tmp3()
    e = 0
    accs = []
    for g in range(n_chains):
        acc = p.tmp3()
        first = True
        for k in range(K):
            if g not in chain_members(k, n_chains):
                continue
            p.op(MUL, acc if first else t, p.ev(e), p.col(SEC_IN, k, _shift(k)))
            e += 1
            if not first:
                p.op(MUL, acc, acc, p.chal(g))
                p.op(ADD, acc, acc, t)
            first = False
        accs.append(acc)
    for g, acc in enumerate(accs):
        p.op(COPY, p.col3(SEC_OUT, 3 * g), acc)
    return Case("chains(%d)" % K, p, K, 3 * n_chains, e)


def combine_store(K1, K2):
    """Two pending forms of K1 and K2 terms on disjoint columns, added and
    stored straight to a COL3 (the compiler's to_col path: no term cap of
    its own between the sum and emit_dot)."""
    p = Program(0)
    t = p.tmp3()
    accs = []
    k = 0
    for n in (K1, K2):
        acc = p.tmp3()
        for i in range(n):
            p.op(MUL, acc if i == 0 else t, p.ev(k), p.col(SEC_IN, k, _shift(k)))
            if i:
                p.op(ADD, acc, acc, t)
            k += 1
        accs.append(acc)
    p.op(ADD, p.col3(SEC_OUT, 0), accs[0], accs[1])
    return Case("combine_store(%d,%d)" % (K1, K2), p, K1 + K2, 3, K1 + K2)


def temp_terms(K):
    """Terms whose sources are row-varying products: col col (a base
    temporary), col3 col3 (an extension temporary, all three components), mixed
    with column terms; more temporaries than a pending form may keep alive
    (MAX_TEMP_REFS), so forms are flushed, and the products arrive unreduced."""
    p = Program(0)
    acc, t, u, v = p.tmp3(), p.tmp3(), p.tmp1(), p.tmp3()
    c = 0
    for k in range(K):
        if k % 4 == 3:
            src = p.col(SEC_IN, c, _shift(k))
            c += 1
        elif k % 2 == 0:
            p.op(MUL, u, p.col(SEC_IN, c, _shift(k)), p.col(SEC_IN, c + 1))
            src = u
            c += 2
        else:
            p.op(MUL, v, p.col3(SEC_IN, c, _shift(k)), p.col3(SEC_IN, c + 3))
            src = v
            c += 6
        p.op(MUL, acc if k == 0 else t, p.ev(k), src)
        if k:
            p.op(ADD, acc, acc, t)
    p.op(COPY, p.col3(SEC_OUT, 0), acc)
    return Case("temp_terms(%d)" % K, p, c, 3, K)


def largest_form(prog, max_terms):
    """Terms of the largest linear form the source program builds when forms
    kept in temporaries are cut at max_terms (the compiler's rule): a plain
    symbolic walk, enough for the builders above (products of two row-varying
    values become one fresh source)."""
    ins, opn = prog.arrays()
    val = {}
    fresh = [0]
    best = 0

    def load(x):
        kind, a, b, c = (int(q) for q in opn[x])
        if kind in (TMP1, TMP3):
            return val.get((kind, a), frozenset())
        if kind == COL:
            return frozenset([(a, b, c)])
        if kind == COL3:
            return frozenset((a, b + j, c) for j in range(3))
        return None  # row constant

    for op, d, a, b in ins.tolist():
        A = load(a)
        B = load(b) if op != COPY else None
        if op == COPY:
            R = A
        elif op == MUL:
            if A is not None and B is not None:
                fresh[0] += 1
                dim = 3 if {int(opn[a][0]), int(opn[b][0])} & {TMP3, COL3} else 1
                R = frozenset(("t", fresh[0], j) for j in range(dim))
            else:
                R = A if B is None else B
        else:
            R = (A or frozenset()) | (B or frozenset())
        R = R or frozenset()
        best = max(best, len(R))
        kind, da = int(opn[d][0]), int(opn[d][1])
        if kind in (TMP1, TMP3):
            if len(R) > max_terms:
                fresh[0] += 1
                R = frozenset(("t", fresh[0], j) for j in range(3 if kind == TMP3 else 1))
            val[(kind, da)] = R
    return best


# ---------------------------------------------------------------- inputs
def rand_canon(rng, shape):
    return rng.integers(0, P, size=shape, dtype=np.uint64)


def make_section(rng, dom, width, worst):
    """Rows 0..255 all A_MAX; rows 256..511 random with one all-A_MAX row per
    wave at lanes 0, 63 and one random lane; the rest random canonical."""
    a = rand_canon(rng, (dom, width))
    if worst:
        a[:256] = A_MAX
        for w0 in range(256, min(512, dom), 64):
            for lane in (0, 63, int(rng.integers(1, 63))):
                a[w0 + lane] = A_MAX
    return a


class Inputs:
    def __init__(self, case, worst, seed, chal_one=None):
        rng = np.random.default_rng(seed)
        dom = 1 << LOG_DOM
        self.dom = dom
        self.S = {k: make_section(rng, dom, w, worst) for k, w in sorted(case.widths.items())}
        self.chal = rand_canon(rng, (8, 3))
        if worst if chal_one is None else chal_one:
            self.chal[:] = (1, 0, 0)
        self.pub = pool_values(rng, N_PUB) if worst else rand_canon(rng, N_PUB)
        self.evals = pool_values(rng, (case.n_ev, 3)) if worst else rand_canon(rng, (case.n_ev, 3))
        # unused by these programs (n domain, no X / xDivXSub / Z_H operands)
        self.x = np.ones(dom, np.uint64)
        self.xdiv = np.zeros((dom, 3), np.uint64)
        self.zh = np.ones(2, np.uint64)

    def sections(self):
        return {k: a.copy() for k, a in self.S.items()}


def oracle_eval(oracle, case, inp, compiled=None, S=None):
    """The oracle's C evaluator on the source program (oc_zxp_eval) or on a
    compiled one (oc_zxc_eval) -> the sections after the run."""
    S = inp.sections() if S is None else S
    secs = (ctypes.c_void_p * 12)()
    strides = np.zeros(12, np.uint64)
    for k, a in S.items():
        secs[k] = a.ctypes.data
        strides[k] = a.shape[1]
    L, p = oracle.lib(), oracle._p
    tail = (ctypes.cast(secs, ctypes.c_void_p), ctypes.c_void_p(strides.ctypes.data), inp.dom, p(inp.chal), p(inp.pub),
            p(inp.evals), p(inp.x), p(inp.xdiv), p(inp.xdiv), p(inp.zh), inp.zh.size)
    if compiled is None:
        ins, opn = case.prog.arrays()
        ins = np.ascontiguousarray(ins, np.uint32)
        opn = np.ascontiguousarray(opn, np.uint32)
        L.oc_zxp_eval(ctypes.c_void_p(ins.ctypes.data), ins.shape[0], ctypes.c_void_p(opn.ctypes.data),
                      max(case.prog.n_tmp1, 1), max(case.prog.n_tmp3, 1), *tail)
    else:
        c = compiled
        ins = np.ascontiguousarray(c["instr"])
        opn = np.ascontiguousarray(c["opnd"])
        term = np.ascontiguousarray(c["term"])
        cst = np.ascontiguousarray(c["cst"]).reshape(-1)
        if cst.size == 0:
            cst = np.zeros(3, np.uint64)
        L.oc_zxc_eval(ctypes.c_void_p(ins.ctypes.data), ins.shape[0], ctypes.c_void_p(opn.ctypes.data), c["n_tmp1"],
                      c["n_tmp3"], ctypes.c_void_p(term.ctypes.data if term.size else 0),
                      ctypes.c_void_p(cst.ctypes.data), *tail)
    return S


def wide_sum_rows(K, dim, inp, rows, cols=None):
    """wide_sum's stored value at the given rows in plain Python integers
    (independent of the oracle); cols replaces the input section."""
    A = inp.S[SEC_IN] if cols is None else cols
    out = []
    for i in rows:
        acc = [0, 0, 0]
        for k in range(K):
            a = int(A[(i + _shift(k)) % inp.dom, k])
            if dim == 3:
                c = [int(x) for x in inp.evals[k]]
            else:
                c = [int(inp.pub[k % N_PUB]) if k % 2 else (POOL[k % len(POOL)] + k) % P, 0, 0]
            for j in range(3):
                acc[j] += c[j] * a
        out.append([x % P for x in acc])
    return out


def fused_fill(src):
    """Largest number of terms any fused-chain accumulator of a printed kernel
    (zkgpu.zxp_jit_source) takes between two reductions, read off the text:
    a loop `for (int q_ ...; q_ < np` adds np terms to every chain whose
    F<g>_0 it feeds, a `.lane(x0_)` block re-seeds chain g with one term."""
    import re
    fill, top, np_ = {}, 0, 0
    for line in src.split("\n"):
        m = re.match(r"for \(int q_ = 0; q_ < (\d+);", line)
        if m:
            np_ = int(m.group(1))
        for g in re.findall(r"F(\d+)_0_\d+ = Dot3\(\); F\d+_0_\d+\.lane\(x0_\)", line):
            fill[g] = 1
        for g in re.findall(r"F(\d+)_0_\d+\.term\(", line):
            fill[g] = fill.get(g, 0) + np_
            top = max(top, fill[g])
    return top
