"""Cases for the three-round power blocks of the Poseidon partial rounds.

csrc/poseidon_perm.hpp evaluates the 22 partial rounds as blocks of textbook
rounds over the original lanes with small integer coefficients
(partial_rounds_pow3; tools/gen_poseidon_sparse.py derive_pow_blocks has the
algebra and the Python model).  This module gives

  * the states the block model and the device permutation are checked on
    (random, all-zero, all p-1, one non-zero lane, states whose first
    partial-round S-box input is 0 or p-1);
  * Dot2::fin, the blocks' two-accumulator reduction, restated in Python
    integers: the words it forms, the conditions of its two carries
    (`fin_mid_carry`, `fin_eps_carry`), inputs built to meet each combination
    (`force_fin`) and the value it must return (`fin_ref`).

tests/test_psb3_cases.py checks all of it on the CPU; tests/test_gpu_psb3.py
runs the same inputs through the library on the GPU.
"""
import importlib.util
import os
import random

P = 0xFFFFFFFF00000001
EPS = 0xFFFFFFFF
M64 = (1 << 64) - 1
W32 = 0xFFFFFFFF

DOT2FIN = 12  # op number of zkgpu_gl_field_selftest_rb_dev (include/zkgpu.h)

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gen_poseidon_sparse",
                                               os.path.join(_ROOT, "tools", "gen_poseidon_sparse.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

RC = gen.load_rc()
PRE = gen.derive(RC)[0]
SCHEDULES = gen.POW_SCHEDULES
KTAB = {name: gen.derive_pow_blocks(RC, sched, PRE) for name, sched in SCHEDULES.items()}


# ------------------------------------------------------------ states
def edge_states():
    """all-zero, all p-1, and for each lane: that lane alone non-zero (1, p-1 and a fixed word)"""
    out = [[0] * 12, [P - 1] * 12]
    for lane in range(12):
        for v in (1, P - 1, 0x0123456789ABCDEF):
            s = [0] * 12
            s[lane] = v
            out.append(s)
    return out


def random_states(n, seed):
    rng = random.Random(seed)
    return [[rng.randrange(P) for _ in range(12)] for _ in range(n)]


def after_full4(st):
    """lanes after the fourth full round's linear layer, the round-4 constants added
    (lane 0 is the first partial round's S-box input)"""
    M = gen.mds()
    st = list(st)
    for r in range(4):
        st = [pow((s + RC[r * 12 + i]) % P, 7, P) for i, s in enumerate(st)]
        st = gen.matvec(M, st)
    return [(s + RC[48 + i]) % P for i, s in enumerate(st)]


_MINV = None
_INV7 = pow(7, -1, P - 1)


def state_with_lane0_after_full4(target, seed):
    """A permutation input whose first partial-round S-box input (lane 0 after four full rounds
    and the round-4 constants) is `target`: the other eleven lanes are drawn at random and the
    four full rounds are run backwards (inverse MDS, seventh roots, constants off)."""
    global _MINV
    if _MINV is None:
        _MINV = gen.inverse(gen.mds())
    rng = random.Random(seed)
    st = [target % P] + [rng.randrange(P) for _ in range(11)]
    st = [(s - RC[48 + i]) % P for i, s in enumerate(st)]
    for r in range(3, -1, -1):
        st = gen.matvec(_MINV, st)
        st = [(pow(s, _INV7, P) - RC[r * 12 + i]) % P for i, s in enumerate(st)]
    return st


# ------------------------------------------------------------ Dot2::fin
def fin_words(L, H):
    """Dot2::fin's words for accumulators L, H (value L + 2^32 H): (lo, h, c1) with
    lo = (mid : L's low word), mid = L's high word + H's low word (carry c1), h = H's high
    word + c1"""
    mid = (L >> 32) + (H & W32)
    c1 = mid >> 32
    h = (H >> 32) + c1
    assert h <= W32  # the device's 32-bit h; holds for every H < 2^63
    return ((mid & W32) << 32) | (L & W32), h, c1


def fin_mid_carry(L, H):
    return fin_words(L, H)[2] == 1


def fin_eps_carry(L, H):
    """the carry of lo + h EPS (selects the + EPS correction)"""
    lo, h, _ = fin_words(L, H)
    return lo + h * EPS > M64


def fin_model(L, H):
    """the device's result word (lazy), step by step"""
    lo, h, _ = fin_words(L, H)
    t = lo + h * EPS
    r = t & M64
    if t >> 64:
        r += EPS
        assert r <= M64  # no second carry
    return r


def fin_ref(L, H):
    return (L + (H << 32)) % P


ACC_MAX = (1 << 58) - 1  # both accumulators of every dot product of the kernels stay below 2^58


WIDE = (1 << 63) - 1  # the largest H the reduction takes (its h stays a 32-bit word); L: any u64


def force_fin(rng, mid_carry, eps_carry, hmax=ACC_MAX):
    """H <= hmax and L <= hmax (kernel range, hmax = ACC_MAX) or any u64 (hmax = WIDE) with the
    mid carry and the EPS carry as asked.  Inside the kernel range both carries cannot meet: a
    mid carry leaves mid < L's high word < 2^26, so lo < 2^58, and h EPS < 2^58 as well."""
    assert not (mid_carry and eps_carry and hmax <= ACC_MAX)
    lmax = hmax if hmax <= ACC_MAX else M64
    for _ in range(1 << 20):
        H = rng.randint(1 << 32, hmax)
        # choose L's high word so that mid carries (or not)
        hl = H & W32
        lim = lmax >> 32
        if mid_carry:
            lo_hi = max(0, (1 << 32) - hl)
            if lo_hi > lim:
                continue
            l1 = rng.randint(lo_hi, lim)
        else:
            l1 = rng.randint(0, min(lim, W32 - hl))
        mid = (l1 + hl) & W32
        h = (H >> 32) + (1 if mid_carry else 0)
        # EPS carry: (mid : l0) + h EPS >= 2^64
        need = (1 << 64) - h * EPS - (mid << 32)  # l0 >= need
        if eps_carry:
            if need > W32:
                continue
            l0 = rng.randint(max(0, need), W32)
        else:
            if need <= 0:
                continue
            l0 = rng.randint(0, min(W32, need - 1))
        L = (l1 << 32) | l0
        if L <= lmax and fin_mid_carry(L, H) == mid_carry and fin_eps_carry(L, H) == eps_carry:
            return L, H
    raise AssertionError("no input found")


def fin_boundary_cases():
    """(name, L, H): the EPS carry exactly at and just below 2^64, zero, the largest kernel
    accumulators and the largest words the op accepts"""
    out = [("zero", 0, 0), ("acc_max", ACC_MAX, ACC_MAX), ("l_max", M64, 0), ("h_only", 0, ACC_MAX),
           ("wide", M64, WIDE)]
    for h in (1, 0x1234, (1 << 26) - 1):
        # no mid carry: H = h 2^32, mid = L's high word; lo + h EPS = 2^64 (carry, r = 0) and 2^64 - 1
        lo = (1 << 64) - h * EPS
        out.append(("eps_at", lo, h << 32))
        out.append(("eps_below", lo - 1, h << 32))
    return out


FIN_COMBOS = [(False, False), (False, True), (True, False), (True, True)]


def fin_cases(rng, per=4):
    """constructed (L, H) pairs: every carry combination inside the kernel range and in the wide
    range, then the boundary cases"""
    out = []
    for mc, ec in FIN_COMBOS:
        for _ in range(per):
            if not (mc and ec):
                out.append(force_fin(rng, mc, ec))
            out.append(force_fin(rng, mc, ec, hmax=WIDE))
    out += [(L, H) for _, L, H in fin_boundary_cases()]
    return out
