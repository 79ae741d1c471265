"""The split of a quotient program's constraint combination into its terms
(zkgpu_zxp_split_constraints, csrc/zxp_split.cpp), restated in Python from the
rule and not from the C++ (tests/test_zxp_split.py, the GPU tests of the
row-list evaluator and of the named constraint check), and the terms on the
CPU oracle: the tapped program run by OracleStark.run over the n-domain
sections.

The rule.  Instructions are walked in order; a TMP3 slot holds a plain value
or a combination {term id: (exponent, negated)}.  CHAL[chal] read as a value is
the new combination {literal 1 at alpha^1}; a product by the operand
CHAL[chal] raises every exponent of a combination by one or makes a plain
value a new term at exponent 1; a sum or difference of a combination and a
plain value x lets x join at exponent 0 (negated when subtracted, all terms
flipped for plain - combination); two combinations unite unless they share a
term; COPY copies.  A combination multiplied by anything else into a TMP3 slot
SPOILS the slot, and so does any instruction that reads a spoiled slot its
TMP3 destination; these instructions are dropped, and the program is refused,
naming the product, only when a spoiled value would count (read with a
combination or CHAL[chal], or written anywhere but to a TMP3 slot).  Terms are
numbered as they join.  One store of a
combination to COL3(SEC_Q_2NS, 0, shift 0), by a COPY or a product by ZI or
the literal 1, fixes every term's exponent and sign; the others are dead."""
import numpy as np

import check_cases as cc
from check_cases import (ADD, CHAL, COL, COL3, COPY, LIT, MUL, P, SEC_Q_2NS, SUB, TMP1, TMP3, ZI, Refused)

ONE = -1  # the value of a read of CHAL[chal]: the literal 1
NOT_ALPHA = "instruction %d multiplies a combination by something other than the combination challenge"


def split(ins, opn, chal=4):
    """-> (tapped instructions (n, 4), tapped operands (m, 4), terms (K, 4): exponent, negated, instr, dead)"""
    ins = [tuple(int(x) for x in r) for r in np.asarray(ins).reshape(-1, 4)]
    opn = [tuple(int(x) for x in r) for r in np.asarray(opn).reshape(-1, 4)]
    n = len(opn)
    if chal >= 8:
        raise Refused("challenge %d out of range" % chal)
    out_i, out_o, joined = [], list(opn), []
    state = {"lit1": None}
    held = {}  # TMP3 slot -> (terms {id: (exponent relative, sign relative)}, exponent shift, sign flip)
    spoiled = {}  # TMP3 slot -> the instruction of the product (by other than alpha) its value derives from
    stored = None

    def spoiled_by(o):
        return spoiled.get(opn[o][1]) if opn[o][0] == TMP3 else None

    def alpha(o):
        return opn[o][0] == CHAL and opn[o][1] == chal

    def held_by(o):
        return held.get(opn[o][1]) if opn[o][0] == TMP3 else None

    def unit(o):
        return opn[o][0] == ZI or opn[o][:3] == (LIT, 1, 0)

    def join(k, x):
        if x == ONE:
            if state["lit1"] is None:
                state["lit1"] = len(out_o)
                out_o.append((LIT, 1, 0, 0))
            x = state["lit1"]
        t = len(joined)
        out_o.append((COL3, SEC_Q_2NS, 3 * t, 0))
        out_i.append((COPY, len(out_o) - 1, x, 0))
        joined.append(k)
        return t

    def fresh(t, e, neg):
        return ({t: (e, neg)}, 0, 0)

    def with_term(c, t, e, neg):
        d, sh, fl = c
        d = dict(d)
        d[t] = (e - sh, neg ^ fl)
        return (d, sh, fl)

    for k, (op, d, a, b) in enumerate(ins):
        if op > COPY or d >= n or a >= n or (op != COPY and b >= n):
            raise Refused("instruction %d out of range" % k)
        sa = spoiled_by(a)
        sb = None if op == COPY else spoiled_by(b)
        if sa is not None or sb is not None:  # only another spoiled value, in a TMP3 slot, may come of it
            origin, other = (sa, b) if sa is not None else (sb, a)
            if opn[d][0] != TMP3 or (op != COPY and (alpha(other) or held_by(other) is not None)):
                raise Refused(NOT_ALPHA % origin)
            held.pop(opn[d][1], None)
            spoiled[opn[d][1]] = origin
            continue
        res, q_form = None, False
        if op == COPY:
            res = fresh(join(k, ONE), 1, 0) if alpha(a) else held_by(a)
            q_form = True
        elif op == MUL and (alpha(a) or alpha(b)):
            other = a if alpha(b) else b
            if alpha(other):
                res = fresh(join(k, ONE), 2, 0)
            elif held_by(other) is not None:
                terms, sh, fl = held_by(other)
                res = (terms, sh + 1, fl)
            else:
                res = fresh(join(k, other), 1, 0)
        elif op == MUL:
            ca, cb = held_by(a), held_by(b)
            if ca is not None or cb is not None:
                if opn[d][0] == TMP3:  # a product the rule does not follow: refused only if it ever counts
                    held.pop(opn[d][1], None)
                    spoiled[opn[d][1]] = k
                    continue
                into_q = opn[d][0] in (COL, COL3) and opn[d][1] == SEC_Q_2NS
                if (ca is not None and cb is not None) or not unit(b if ca is not None else a) or not into_q:
                    raise Refused(NOT_ALPHA % k)
                res, q_form = (ca if ca is not None else cb), True
        else:
            ca, cb = held_by(a), held_by(b)
            if alpha(a):
                ca = fresh(join(k, ONE), 1, 0)
            if alpha(b):
                cb = fresh(join(k, ONE), 1, 0)
            if ca is not None or cb is not None:
                res = ca
                if cb is not None:
                    terms, sh, fl = cb
                    if op == SUB:
                        fl ^= 1
                    if res is None:
                        res = (terms, sh, fl)
                    else:
                        for t, (e, s) in terms.items():  # (in the order they joined the second)
                            if t in res[0]:
                                raise Refused("instruction %d combines two combinations that share term %d" % (k, t))
                            res = with_term(res, t, e + sh, s ^ fl)
                if ca is None:
                    res = with_term(res, join(k, a), 0, 0)
                if cb is None:
                    res = with_term(res, join(k, b), 0, 1 if op == SUB else 0)
        kind, sec, col, shift = opn[d]
        to_q = kind in (COL, COL3) and sec == SEC_Q_2NS
        if res is None:
            if to_q:
                raise Refused("instruction %d stores a value free of the combination challenge to SEC_Q_2NS" % k)
            if kind == TMP3:
                held.pop(sec, None)
                spoiled.pop(sec, None)
            out_i.append((op, d, a, b))
        elif kind == TMP3:
            spoiled.pop(sec, None)
            held[sec] = res
        elif kind == TMP1:
            raise Refused("instruction %d writes a combination to a TMP1 slot" % k)
        elif kind in (COL, COL3):
            if (kind, sec, col, shift) != (COL3, SEC_Q_2NS, 0, 0):
                raise Refused("instruction %d stores a combination to a column other than q (SEC_Q_2NS, column 0, "
                              "shift 0)" % k)
            if not q_form:
                raise Refused("instruction %d stores a combination to q other than by a COPY or a product by ZI or 1"
                              % k)
            if stored is not None:
                raise Refused("instruction %d is a second store to q" % k)
            stored = res
        else:
            raise Refused("instruction %d writes a combination to an operand of kind %d" % (k, kind))
    if stored is None:
        raise Refused("no combination is stored to SEC_Q_2NS")
    terms, sh, fl = stored
    table = [(terms[t][0] + sh, terms[t][1] ^ fl, k, 0) if t in terms else (0, 0, k, 1) for t, k in enumerate(joined)]
    return (np.array(out_i, np.uint32).reshape(-1, 4), np.array(out_o, np.uint32).reshape(-1, 4),
            np.array(table, np.uint32).reshape(-1, 4))


class TappedProgram:
    """what OracleStark.run and zkgpu.zxp_eval_rows_dev take: the tapped n-domain step42ns"""

    def __init__(self, prog, extend_bits, chal=4, split=None):
        """split: what takes (ins, opn, chal) apart -- the restatement above, or the library's
        zkgpu.zxp_split_constraints"""
        nd = cc.NDomainProgram(prog, extend_bits)
        self.ins, self.opn, self.terms = (split or globals()["split"])(nd.ins, nd.opn, chal)
        self.domain_ext = 0
        self.n_tmp1, self.n_tmp3 = prog.n_tmp1, prog.n_tmp3

    def arrays(self):
        return np.ascontiguousarray(self.ins), np.ascontiguousarray(self.opn)


def oracle_terms(ostark, alpha, split=None):
    """After ostark.prove(): (the term table, v: (N, K, 3) canonical values of
    every term of step42ns's combination on the n domain with challenge 4 = alpha)"""
    inst = ostark.inst
    tp = TappedProgram(inst.programs["step42ns"], inst.blowup_bits, split=split)
    k = tp.terms.shape[0]
    ostark.S[SEC_Q_2NS] = np.zeros((ostark.N, 3 * max(k, 1)), np.uint64)
    ch = np.array(ostark.challenges, np.uint64).reshape(8, 3).copy()
    ch[4] = np.array([int(a) % P for a in alpha], np.uint64)
    ostark.run(tp, ch, np.zeros(3, np.uint64))
    v = (ostark.S[SEC_Q_2NS] % np.uint64(P)).reshape(ostark.N, max(k, 1), 3)[:, :k].copy()
    return tp.terms, v


def named(terms, v, row):
    """(ids, values) of the live terms that are not zero at this row, ascending"""
    ids = [t for t in range(terms.shape[0]) if not terms[t, 3] and v[row, t].any()]
    return ids, [[int(x) for x in v[row, t]] for t in ids]


def mul3(a, b):
    """F_p^3 = F_p[x] / (x^3 - x - 1)"""
    a0, a1, a2 = a
    b0, b1, b2 = b
    c0, c1, c2, c3, c4 = a0 * b0, a0 * b1 + a1 * b0, a0 * b2 + a1 * b1 + a2 * b0, a1 * b2 + a2 * b1, a2 * b2
    # x^3 = x + 1, x^4 = x^2 + x
    return [(c0 + c3) % P, (c1 + c3 + c4) % P, (c2 + c4) % P]


def combine(terms, values, alpha, ids=None):
    """sum over the given (default: all live) terms of (-1)^negated * alpha^exponent * value, as 3 ints"""
    alpha = [int(a) % P for a in alpha]
    ids = [t for t in range(terms.shape[0]) if not terms[t, 3]] if ids is None else ids
    top = max([int(terms[t, 0]) for t in ids] + [0])
    pw = [[1, 0, 0]]
    for _ in range(top):
        pw.append(mul3(pw[-1], alpha))
    acc = [0, 0, 0]
    for t, val in zip(ids, values):
        m = mul3(pw[int(terms[t, 0])], [int(x) for x in val])
        sign = -1 if terms[t, 1] else 1
        acc = [(x + sign * y) % P for x, y in zip(acc, m)]
    return acc
