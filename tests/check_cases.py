"""The constraint check's cases (tests/test_zxp_n_domain.py, tests/test_gpu_constraint_check.py).

A Python restatement of the rewrite of a quotient program onto the trace
domain (zkgpu_zxp_to_n_domain, csrc/zxp_n_domain.cpp), written from the rules
and not from the C++, and the check itself on the CPU oracle: the restated
program over the n-domain sections an OracleStark holds after prove()."""
import numpy as np

P = 0xFFFFFFFF00000001
TMP1, TMP3, COL, COL3, LIT, CHAL, PUB, X, EVAL, XDIV, XDIVW, ZI = range(12)
ADD, SUB, MUL, COPY = range(4)
(SEC_CM1_N, SEC_CM2_N, SEC_CM3_N, SEC_TMP_N, SEC_CONST_N, SEC_CM1_2NS, SEC_CM2_2NS, SEC_CM3_2NS, SEC_CM4_2NS,
 SEC_CONST_2NS, SEC_Q_2NS, SEC_F_2NS) = range(12)
TO_N = {SEC_CM1_2NS: SEC_CM1_N, SEC_CM2_2NS: SEC_CM2_N, SEC_CM3_2NS: SEC_CM3_N, SEC_CONST_2NS: SEC_CONST_N}
MAX_ROWS = 16


class Refused(Exception):
    pass


def _s32(v):
    v = int(v) & 0xFFFFFFFF
    return v - (1 << 32) if v >> 31 else v


def to_n_domain(ins, opn, extend_bits):
    """the rewritten operand table (n_opnd x 4, uint32) or Refused"""
    ins = [tuple(int(x) for x in r) for r in np.asarray(ins).reshape(-1, 4)]
    opn = [tuple(int(x) for x in r) for r in np.asarray(opn).reshape(-1, 4)]
    n = len(opn)
    src, dst = set(), set()
    for k, (op, d, a, b) in enumerate(ins):
        if op > COPY or d >= n or a >= n or (op != COPY and b >= n):
            raise Refused("instruction %d out of range" % k)
        dst.add(d)
        src.add(a)
        if op != COPY:
            src.add(b)

    def is_q(k):
        return opn[k][0] in (COL, COL3) and opn[k][1] == SEC_Q_2NS

    zi_products = 0
    for k, (op, d, a, b) in enumerate(ins):
        uses = [opn[a][0] == ZI] + ([opn[b][0] == ZI] if op != COPY else [])
        if opn[d][0] == ZI:
            raise Refused("instruction %d writes ZI" % k)
        if not any(uses):
            continue
        if op != MUL or not is_q(d) or all(uses):
            raise Refused("instruction %d uses ZI other than as a factor of a product stored to SEC_Q_2NS" % k)
        zi_products += 1
    if not zi_products:
        raise Refused("no product by ZI is stored to SEC_Q_2NS")
    out = []
    for k, (kind, a, b, c) in enumerate(opn):
        if kind in (TMP1, TMP3, LIT, CHAL, PUB, X):
            out.append((kind, a, b, c))
        elif kind == ZI:
            out.append((LIT, 1, 0, 0))
        elif kind in (COL, COL3):
            sh = _s32(c)
            if a == SEC_Q_2NS:
                if k in src:
                    raise Refused("operand %d reads SEC_Q_2NS" % k)
                if sh:
                    raise Refused("operand %d stores to SEC_Q_2NS at row shift %d" % (k, sh))
                out.append((kind, a, b, c))
                continue
            if a not in TO_N:
                raise Refused("operand %d names section %d" % (k, a))
            if k in dst:
                raise Refused("operand %d stores to section %d" % (k, a))
            if sh % (1 << extend_bits):
                raise Refused("operand %d: row shift %d is no multiple of %d" % (k, sh, 1 << extend_bits))
            out.append((kind, TO_N[a], b, (sh >> extend_bits) & 0xFFFFFFFF))
        else:
            raise Refused("operand %d of kind %d" % (k, kind))
    return np.array(out, np.uint32).reshape(-1, 4)


class NDomainProgram:
    """what OracleStark.run takes: step42ns with its operands rewritten"""

    def __init__(self, prog, extend_bits):
        self.ins, opn = prog.arrays()
        self.opn = to_n_domain(self.ins, opn, extend_bits)
        self.domain_ext = 0
        self.n_tmp1, self.n_tmp3 = prog.n_tmp1, prog.n_tmp3

    def arrays(self):
        return np.ascontiguousarray(self.ins), np.ascontiguousarray(self.opn)


def oracle_check(ostark, alpha):
    """After ostark.prove(): the constraint combination C of step42ns on the
    n domain with challenge 4 = alpha -> (n_bad, the lowest 16 failing rows,
    C at the first as 3 ints; [0, 0, 0] when none fails)"""
    inst = ostark.inst
    ostark.S[SEC_Q_2NS] = np.zeros((ostark.N, 3), np.uint64)
    ch = np.array(ostark.challenges, np.uint64).reshape(8, 3).copy()
    ch[4] = np.array([int(a) % P for a in alpha], np.uint64)
    ostark.run(NDomainProgram(inst.programs["step42ns"], inst.blowup_bits), ch, np.zeros(3, np.uint64))
    c = ostark.S[SEC_Q_2NS] % np.uint64(P)
    bad = np.flatnonzero(c.any(axis=1))
    value = [int(v) for v in c[bad[0]]] if bad.size else [0, 0, 0]
    return int(bad.size), [int(r) for r in bad[:MAX_ROWS]], value


def corrupt(ostark, rows):
    """a2 of triple 0 (cm1 column 2: in no plookup, and the grand products
    telescope, so the proof still completes) + 1 at these rows, after witness()"""
    for r in rows:
        ostark.S[0][r, 2] = (int(ostark.S[0][r, 2]) + 1) % P
