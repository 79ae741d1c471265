#!/usr/bin/env python3
"""Derive the sparse partial-round form of Poseidon-GL and emit it as a header.

The reference evaluates the permutation in its textbook form
(`poseidon_g_executor.cpp:201-231`): every one of the 22 partial rounds adds a
12-lane constant, applies x^7 to lane 0 and multiplies by the 12x12 MDS.  The
same permutation can be rewritten exactly (Poseidon paper, appendix B:
"optimised partial rounds") so that

    s += PRE                  (full 12-lane constant, once)
    s[1..11] = D0 * s[1..11]  (dense 11x11 "initial matrix", once)
    for k in 0..21:
        s0 = s0^7 ; s0 += POST[k]             (POST[21] = 0)
        s0' = 25*s0 + <W[k], s[1..11]> ; s[j] += V[k][j] * s0   (sparse S_k)

Derivation (all arithmetic mod p):
  * constants: walking backwards, the lanes-1..11 part of a round constant
    commutes with the lane-0 S-box, and a vector added after round k-1's MDS
    equals M^-1 times it added before that MDS; lane 0 of what crosses an
    S-box stays behind as POST.  Only round 0 keeps a full vector (PRE).
  * matrices: any N with block form [[n00, w^T], [v, N^]] factors as
    S * D with D = diag(1, N^) applied first and
    S = [[n00, (N^-T w)^T], [v, I]].  D touches lanes 1..11 only, so it
    commutes with the lane-0 S-box and constant and folds into the previous
    round's matrix; after 22 steps the leftover D is the initial matrix.
    Row 0 is never changed, so n00 stays MDS[0][0] = 25 (small).

The input is the product's committed round-constant header (data from the
reference's table); the result is checked here against the textbook form on
random states before anything is written.  Output:
  zkevm-prover_amd/csrc/poseidon_gl_sparse.h

Usage: python tools/gen_poseidon_sparse.py
"""
import os
import random
import re

P = 0xFFFFFFFF00000001
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MCIRC = [17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20]
MDIAG = [8] + [0] * 11
RF_HALF, RP = 4, 22


def load_rc():
    text = open(os.path.join(ROOT, "zkevm-prover_amd/csrc/poseidon_gl_constants.h")).read()
    vals = [int(t, 16) for t in re.findall(r"0x([0-9a-f]{16})ULL", text)]
    assert len(vals) == 360
    return vals


def mds():
    return [[(MCIRC[(y - x) % 12] + (MDIAG[x] if x == y else 0)) for y in range(12)] for x in range(12)]


def matmul(a, b):
    n, m, k = len(a), len(b[0]), len(b)
    return [[sum(a[i][t] * b[t][j] for t in range(k)) % P for j in range(m)] for i in range(n)]


def matvec(a, v):
    return [sum(a[i][t] * v[t] for t in range(len(v))) % P for i in range(len(a))]


def transpose(a):
    return [list(r) for r in zip(*a)]


def inverse(a):
    n = len(a)
    m = [list(r) + [1 if i == j else 0 for j in range(n)] for i, r in enumerate(a)]
    for c in range(n):
        piv = next(r for r in range(c, n) if m[r][c] % P)
        m[c], m[piv] = m[piv], m[c]
        inv = pow(m[c][c], P - 2, P)
        m[c] = [x * inv % P for x in m[c]]
        for r in range(n):
            if r != c and m[r][c]:
                f = m[r][c]
                m[r] = [(x - f * y) % P for x, y in zip(m[r], m[c])]
    return [r[n:] for r in m]


def perm_textbook(st, rc):
    M = mds()
    st = list(st)
    for r in range(2 * RF_HALF + RP):
        st = [(s + rc[r * 12 + i]) % P for i, s in enumerate(st)]
        if r < RF_HALF or r >= RF_HALF + RP:
            st = [pow(s, 7, P) for s in st]
        else:
            st[0] = pow(st[0], 7, P)
        st = matvec(M, st)
    return st


def derive(rc):
    M = mds()
    Minv = inverse(M)
    # constants (backwards over the partial rounds)
    carry = [0] * 12
    post = [0] * RP
    pre = None
    for k in range(RP - 1, -1, -1):
        c = rc[(RF_HALF + k) * 12:(RF_HALF + k + 1) * 12]
        post[k] = carry[0]
        full = [(c[i] + (carry[i] if i else 0)) % P for i in range(12)]
        if k > 0:
            carry = matvec(Minv, full)
        else:
            pre = full
    # matrices (backwards)
    W, V = [None] * RP, [None] * RP
    N = M
    for k in range(RP - 1, -1, -1):
        n00 = N[0][0]
        w = N[0][1:]
        v = [N[i][0] for i in range(1, 12)]
        Nh = [row[1:] for row in N[1:]]
        assert n00 == M[0][0]
        what = matvec(transpose(inverse(Nh)), w)
        W[k], V[k] = what, v
        D = [[1] + [0] * 11] + [[0] + Nh[i] for i in range(11)]
        N = matmul(D, M) if k > 0 else None
        if k == 0:
            D0 = Nh
    return pre, post, D0, W, V


def perm_sparse(st, rc, pre, post, D0, W, V):
    M = mds()
    st = list(st)
    for r in range(RF_HALF):
        st = [pow((s + rc[r * 12 + i]) % P, 7, P) for i, s in enumerate(st)]
        st = matvec(M, st)
    st = [(s + pre[i]) % P for i, s in enumerate(st)]
    st = [st[0]] + matvec(D0, st[1:])
    for k in range(RP):
        s0 = (pow(st[0], 7, P) + post[k]) % P
        n0 = (M[0][0] * s0 + sum(W[k][j] * st[1 + j] for j in range(11))) % P
        st = [n0] + [(st[1 + j] + V[k][j] * s0) % P for j in range(11)]
    for r in range(RF_HALF + RP, 2 * RF_HALF + RP):
        st = [pow((s + rc[r * 12 + i]) % P, 7, P) for i, s in enumerate(st)]
        st = matvec(M, st)
    return st


BLOCK = 11  # partial rounds per block of the device evaluator


def limbs6(c):
    """Coefficient c as 6 u32 limbs: 22/21/21-bit limbs of c and of c*2^32 mod p.
    A lazy lane a = a0 + a1*2^32 times c == a0*c + a1*(c*2^32): both products land
    in the same three accumulators of weight 2^0, 2^22, 2^43."""
    c %= P
    c2 = c * (1 << 32) % P
    return [c & 0x3FFFFF, (c >> 22) & 0x1FFFFF, c >> 43, c2 & 0x3FFFFF, (c2 >> 22) & 0x1FFFFF, c2 >> 43]


def limbs3(k):
    k %= P
    return [k & 0x3FFFFF, (k >> 22) & 0x1FFFFF, k >> 43]


def derive_blocks(rc, pre, post, D0, W, V):
    """Dot-product form of the partial rounds used by the device code.

    Device state after the first four full rounds (whose last MDS already added
    PRE): x = lane 0, L = D0 * lanes[1..11] (materialised).  Per block of
    BLOCK rounds k = k0..k0+BLOCK-1 with y_k = x_k^7 (raw S-box output,
    s0_k = y_k + POST[k]):
        x_{k+1} = 25 s0_k + W_k . L(k0) + sum_{k0<=i<k} (W_k . V_i) s0_i
        L(k0+BLOCK) = L(k0) + sum_i V_i s0_i
    Every POST term and, in the last block, the round-26 constants are folded
    into per-dot constant offsets.  Returns (d0_table, block_tables), u32 lists.
    """
    M = mds()
    c26 = rc[(RF_HALF + RP) * 12:(RF_HALF + RP + 1) * 12]
    d0 = []
    for i in range(11):
        d0 += limbs3(0)
        for j in range(11):
            d0 += limbs6(D0[i][j])
    blocks = []
    for b in range(RP // BLOCK):
        k0 = b * BLOCK
        last = b == RP // BLOCK - 1
        t = []
        for tt in range(BLOCK):
            k = k0 + tt
            coef_y = {k: M[0][0]}
            for i in range(k0, k):
                coef_y[i] = sum(W[k][j] * V[i][j] for j in range(11)) % P
            const = sum(cy * post[i] for i, cy in coef_y.items()) % P
            if last and tt == BLOCK - 1:
                const = (const + c26[0]) % P
            t += limbs3(const)
            t += limbs6(coef_y[k])
            for j in range(11):
                t += limbs6(W[k][j])
            for i in range(k0, k):
                t += limbs6(coef_y[i])
        for j in range(11):
            const = sum(V[i][j] * post[i] for i in range(k0, k0 + BLOCK)) % P
            if last:
                const = (const + c26[1 + j]) % P
            t += limbs3(const)
            for i in range(k0, k0 + BLOCK):
                t += limbs6(V[i][j])
        blocks.append(t)
    assert all(len(x) == len(blocks[0]) for x in blocks)
    return d0, blocks


def perm_blocks(st, rc, pre, d0, blocks):
    """Evaluate the permutation exactly as the device code does (tables only)."""
    M = mds()
    st = [(s + rc[i]) % P for i, s in enumerate(st)]
    for r in range(RF_HALF):
        st = [pow(s, 7, P) for s in st]
        st = matvec(M, st)
        nxt = rc[(r + 1) * 12:(r + 2) * 12] if r < RF_HALF - 1 else pre
        st = [(s + c) % P for s, c in zip(st, nxt)]

    def coef(l6):
        return (l6[0] + (l6[1] << 22) + (l6[2] << 43)) % P

    def const(l3):
        return (l3[0] + (l3[1] << 22) + (l3[2] << 43)) % P

    x = st[0]
    L = []
    for i in range(11):
        base = i * 69
        L.append((const(d0[base:base + 3]) + sum(coef(d0[base + 3 + 6 * j:base + 9 + 6 * j]) * st[1 + j]
                                                   for j in range(11))) % P)
    for tb in blocks:
        pos = 0
        ys = []
        for tt in range(BLOCK):
            y = pow(x, 7, P)
            ys.append(y)
            acc = const(tb[pos:pos + 3]); pos += 3
            acc += coef(tb[pos:pos + 6]) * y; pos += 6
            for j in range(11):
                acc += coef(tb[pos:pos + 6]) * L[j]; pos += 6
            for i in range(tt):
                acc += coef(tb[pos:pos + 6]) * ys[i]; pos += 6
            x = acc % P
        newL = []
        for j in range(11):
            acc = const(tb[pos:pos + 3]) + L[j]; pos += 3
            for i in range(BLOCK):
                acc += coef(tb[pos:pos + 6]) * ys[i]; pos += 6
            newL.append(acc % P)
        L = newL
    st = [x] + L
    for r in range(RF_HALF + RP, 2 * RF_HALF + RP):
        st = [pow(s, 7, P) for s in st]
        st = matvec(M, st)
        if r < 2 * RF_HALF + RP - 1:
            st = [(s + c) % P for s, c in zip(st, rc[(r + 1) * 12:(r + 2) * 12])]
    return st


# ---------------------------------------------------------------- power blocks
# Partial rounds as blocks of up to three TEXTBOOK rounds over the original
# lanes.  With s the lanes at block start (the block's first round constants
# already added), Z = diag(0, 1, .., 1) and y_i the S-box output of round i:
#     s_y = s with lane 0 replaced by y0 = s[0]^7
#     u1 = (P1 s_y)[0] + K1                               y1 = u1^7
#     u2 = (P2 s_y)[0] + P1[0][0] y1 + K2                 y2 = u2^7
#     s' = P3 s_y + (P2 e0) y1 + (P1 e0) y2 + K3
#     P1 = M,  P2 = M Z M,  P3 = M Z M Z M
# Z drops the lane-0 value that the next S-box replaces, so the S-box outputs
# enter as themselves (no u^7 - u differences, no subtraction) and every
# coefficient is a non-negative integer <= the matching entry of M, M^2, M^3
# (< 2^21): a lane's 32-bit halves times a coefficient sum carry-free in two
# u64 accumulators.  A block of n < 3 rounds stops at P_n.
POW_SCHEDULES = {"7x3+1": [3] * 7 + [1], "6x3+2x2": [3] * 6 + [2, 2]}
POW_SCHEDULE = "7x3+1"  # the device code's (csrc/poseidon_perm.hpp partial_rounds_pow3)


def pow_mats():
    """[P1, P2, P3] as plain integers (never reduced: they stay < 2^21)."""
    M = mds()

    def zmul(a, b):  # a Z b
        return [[sum(a[i][t] * b[t][j] for t in range(1, 12)) for j in range(12)] for i in range(12)]

    P1 = M
    P2 = zmul(M, P1)
    P3 = zmul(M, P2)
    return [P1, P2, P3]


def pow_block_rows(n):
    """The dot products of an n-round block, in evaluation order: (kind, row, coefficients) with
    kind 'u' (the next S-box input, row 0 of P_i) or 's' (output lane `row`); the coefficients
    multiply s_y[0..11], then y1 .. (as many as are known)."""
    Pm = pow_mats()
    rows = []
    for i in range(1, n):
        rows.append(("u", i, Pm[i - 1][0] + [Pm[i - m - 1][0][0] for m in range(1, i)]))
    for x in range(12):
        rows.append(("s", x, Pm[n - 1][x] + [Pm[n - m - 1][x][0] for m in range(1, n)]))
    return rows


def pow_acc_bound(n):
    """Largest value either u64 accumulator of an n-round block can reach for arbitrary u64
    lanes and S-box outputs: the 32-bit seed plus (2^32 - 1) times the row's coefficient sum."""
    return max((1 << 32) - 1 + ((1 << 32) - 1) * sum(c) for _, _, c in pow_block_rows(n))


def derive_pow_blocks(rc, schedule, pre=None):
    """Per-block constants of the power-block form for a schedule (block lengths summing to RP).

    The first block's input carries PRE (what the fourth full round's linear layer adds
    today), not the plain round-4 constants: PRE - c_4 is a constant vector whose lane 0 is
    zero, and its image under P1, P2, P3 is taken out of the first block's constants.  Every
    block's last constant vector holds the next round's constants, the last block's the
    round-26 ones.  Returns a list of blocks, each a list of u32: for i < n the low and high
    half of K_i, then the 12 (low, high) pairs of the vector K_n -- the seeds of the two
    accumulators of each dot product."""
    assert sum(schedule) == RP and all(1 <= n <= 3 for n in schedule)
    if pre is None:
        pre = derive(rc)[0]
    M = mds()
    c4 = rc[RF_HALF * 12:(RF_HALF + 1) * 12]
    assert pre[0] == c4[0]
    k = [0] + [(c4[i] - pre[i]) % P for i in range(1, 12)]  # true lanes = given lanes + k
    out = []
    r = RF_HALF
    for n in schedule:
        assert pow_acc_bound(n) < 1 << 64
        words = []
        for i in range(1, n + 1):
            full = [(v + c) % P for v, c in zip(matvec(M, k), rc[(r + i) * 12:(r + i + 1) * 12])]
            if i < n:
                words += [full[0] & 0xFFFFFFFF, full[0] >> 32]
                k = [0] + full[1:]
            else:
                for v in full:
                    words += [v & 0xFFFFFFFF, v >> 32]
        k = [0] * 12
        r += n
        out.append(words)
    return out


def pow_block_eval(s, words, n, check=None):
    """One n-round block exactly as the device evaluates it: integer accumulators, reduced
    once per dot product.  s: any u64 lanes.  check(lo, hi) sees every accumulator pair."""
    y = [pow(s[0], 7, P)]
    sy = [y[0]] + list(s[1:])
    pos = 0
    res = []
    for kind, _, coef in pow_block_rows(n):
        vals = sy + y[1:]
        assert len(vals) == len(coef)
        lo = words[pos] + sum((v & 0xFFFFFFFF) * c for v, c in zip(vals, coef))
        hi = words[pos + 1] + sum((v >> 32) * c for v, c in zip(vals, coef))
        pos += 2
        if check:
            check(lo, hi)
        v = (lo + (hi << 32)) % P
        if kind == "u":
            y.append(pow(v, 7, P))
        else:
            res.append(v)
    assert pos == len(words)
    return res


def perm_pow_blocks(st, rc, pre, schedule, ktab, check=None):
    """The permutation with the partial rounds in power-block form (tables only)."""
    M = mds()
    st = [(s + rc[i]) % P for i, s in enumerate(st)]
    for r in range(RF_HALF):
        st = [pow(s, 7, P) for s in st]
        st = matvec(M, st)
        nxt = rc[(r + 1) * 12:(r + 2) * 12] if r < RF_HALF - 1 else pre
        st = [(s + c) % P for s, c in zip(st, nxt)]
    for n, words in zip(schedule, ktab):
        st = pow_block_eval(st, words, n, check)
    for r in range(RF_HALF + RP, 2 * RF_HALF + RP):
        st = [pow(s, 7, P) for s in st]
        st = matvec(M, st)
        if r < 2 * RF_HALF + RP - 1:
            st = [(s + c) % P for s, c in zip(st, rc[(r + 1) * 12:(r + 2) * 12])]
    return st


def emit_pow(rc, pre):
    """Header lines of the device schedule: the three-round blocks' seeds and the constants of
    the single round left over (the plain round-26 constants: it is one textbook round)."""
    sched = POW_SCHEDULES[POW_SCHEDULE]
    assert sched[:-1] == [3] * (len(sched) - 1) and sched[-1] == 1
    ktab = derive_pow_blocks(rc, sched, pre)
    tail = [lo | (hi << 32) for lo, hi in zip(ktab[-1][0::2], ktab[-1][1::2])]
    assert tail == rc[(RF_HALF + RP) * 12:(RF_HALF + RP + 1) * 12]
    flat = [w for t in ktab[:-1] for w in t]
    lines = ["// power-block form (see derive_pow_blocks), schedule %s: per three-round block the" % POW_SCHEDULE,
             "// accumulator seeds K1, K2 (low, high half) and K3[0..11] (low, high pairs), u32",
             f"#define ZKGPU_PSB3_NBLOCKS {len(ktab) - 1}",
             f"#define ZKGPU_PSB3_BLOCK_WORDS {len(ktab[0])}",
             f"static constexpr uint32_t ZKGPU_PSB3_K[{len(flat)}] = {{"]
    for i in range(0, len(flat), 8):
        lines.append("    " + ", ".join(f"0x{v:08x}u" for v in flat[i:i + 8]) + ",")
    lines.append("};")
    return lines


def emit_pow_alt(path, rc, pre):
    """The other schedule's seeds, for the isolated benchmark's variant only
    (tools/poseidon_bench.hip): six three-round blocks, then two two-round blocks."""
    sched = POW_SCHEDULES["6x3+2x2"]
    ktab = derive_pow_blocks(rc, sched, pre)
    lines = ["// GENERATED by tools/gen_poseidon_sparse.py -- do not edit.",
             "// Power-block seeds of the 6x3+2x2 schedule (benchmark variant; the kernels use",
             "// csrc/poseidon_gl_sparse.h ZKGPU_PSB3_K).  Per block: K_i (low, high) for i < n, then K_n[0..11].",
             "#pragma once", "#include <stdint.h>"]
    for name, n in (("PSB_ALT_K3", 3), ("PSB_ALT_K2", 2)):
        flat = [w for nn, t in zip(sched, ktab) if nn == n for w in t]
        lines.append(f"static constexpr uint32_t {name}[{len(flat)}] = {{")
        for i in range(0, len(flat), 8):
            lines.append("    " + ", ".join(f"0x{v:08x}u" for v in flat[i:i + 8]) + ",")
        lines.append("};")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def emit(path, pre, post, D0, W, V, d0tab=None, btabs=None, cap0=None, pow_lines=None):
    def arr(name, vals, per=4):
        out = [f"static constexpr uint64_t {name}[{len(vals)}] = {{"]
        for i in range(0, len(vals), per):
            out.append("    " + ", ".join(f"0x{v:016x}ULL" for v in vals[i:i + per]) + ",")
        out.append("};")
        return out

    lines = [
        "// GENERATED by tools/gen_poseidon_sparse.py -- do not edit.",
        "// Poseidon-GL partial rounds in sparse form (exactly equal to the textbook",
        "// permutation of poseidon_g_executor.cpp:201-231; see the generator's docstring).",
        "#ifndef ZKGPU_POSEIDON_GL_SPARSE_H",
        "#define ZKGPU_POSEIDON_GL_SPARSE_H",
        "#include <stdint.h>",
        "// full constant added once before the partial rounds",
    ]
    lines += arr("ZKGPU_PSP_PRE", pre)
    lines += ["// lane-0 constant added after the S-box of partial round k"]
    lines += arr("ZKGPU_PSP_POST", post)
    lines += ["// dense 11x11 initial matrix on lanes 1..11, row-major"]
    lines += arr("ZKGPU_PSP_D0", [x for r in D0 for x in r])
    lines += ["// row 0 of S_k (lanes 1..11): s0' = 25*s0 + sum W[k][j] s[1+j]"]
    lines += arr("ZKGPU_PSP_W", [x for r in W for x in r])
    lines += ["// column 0 of S_k: s[1+j] += V[k][j] * s0"]
    lines += arr("ZKGPU_PSP_V", [x for r in V for x in r])
    if d0tab is not None:
        def arr32(name, vals, per=12):
            out = [f"static constexpr uint32_t {name}[{len(vals)}] = {{"]
            for i in range(0, len(vals), per):
                out.append("    " + ", ".join(f"0x{v:06x}u" for v in vals[i:i + per]) + ",")
            out.append("};")
            return out
        lines += ["// device block form (see derive_blocks): limb tables, u32",
                  f"#define ZKGPU_PSB_BLOCK {BLOCK}",
                  f"#define ZKGPU_PSB_NBLOCKS {len(btabs)}",
                  f"#define ZKGPU_PSB_BLOCK_WORDS {len(btabs[0])}"]
        lines += arr32("ZKGPU_PSB_D0", d0tab)
        lines += arr32("ZKGPU_PSB_BLOCKS", [w for t in btabs for w in t])
    if cap0 is not None:
        lines += ["// round 0 of a state whose lanes 8..11 enter as zero: their S-box outputs",
                  "// (0 + RC[8 + k])^7 through the linear layer, plus the round-1 constants:",
                  "// K[x] = RC[12 + x] + sum_k M[x][8 + k] RC[8 + k]^7"]
        lines += arr("ZKGPU_PS_CAP0_K", cap0)
    if pow_lines is not None:
        lines += pow_lines
    lines += ["#endif  // ZKGPU_POSEIDON_GL_SPARSE_H", ""]
    with open(path, "w") as f:
        f.write("\n".join(lines))


def main():
    rc = load_rc()
    pre, post, D0, W, V = derive(rc)
    assert post[RP - 1] == 0
    rnd = random.Random(12)
    for _ in range(64):
        st = [rnd.randrange(P) for _ in range(12)]
        assert perm_sparse(st, rc, pre, post, D0, W, V) == perm_textbook(st, rc)
    d0tab, btabs = derive_blocks(rc, pre, post, D0, W, V)
    for _ in range(16):
        st = [rnd.randrange(P) for _ in range(12)]
        assert perm_blocks(st, rc, pre, d0tab, btabs) == perm_textbook(st, rc)
    # a state whose lanes 8..11 are zero (a tree node, a sponge's first block):
    # their round-0 S-boxes see the round constants alone
    # alone: a constant vector through the linear layer, folded into the
    # round-1 constants
    M = mds()
    sbox = [pow(rc[8 + k], 7, P) for k in range(4)]
    cap0 = [(rc[12 + x] + sum(M[x][8 + k] * sbox[k] for k in range(4))) % P for x in range(12)]
    for _ in range(16):
        st = [rnd.randrange(P) for _ in range(8)] + [0] * 4
        r0 = [pow((s + c) % P, 7, P) for s, c in zip(st, rc[:12])]
        full = [(v + c) % P for v, c in zip(matvec(M, r0), rc[12:24])]
        assert full == [(v + c) % P for v, c in zip(matvec(M, r0[:8] + [0] * 4), cap0)]
    # power blocks: both schedules against the textbook form, every accumulator below 2^64
    def below_2_64(lo, hi):
        assert lo < 1 << 64 and hi < 1 << 64
    for sched in POW_SCHEDULES.values():
        ktab = derive_pow_blocks(rc, sched, pre)
        for _ in range(16):
            st = [rnd.randrange(P) for _ in range(12)]
            assert perm_pow_blocks(st, rc, pre, sched, ktab, below_2_64) == perm_textbook(st, rc)
    emit(os.path.join(ROOT, "zkevm-prover_amd/csrc/poseidon_gl_sparse.h"), pre, post, D0, W, V, d0tab, btabs, cap0,
         emit_pow(rc, pre))
    emit_pow_alt(os.path.join(ROOT, "tools/poseidon_bench_alt.h"), rc, pre)
    print("sparse, block and power-block forms verified on random states; header written")


if __name__ == "__main__":
    main()
