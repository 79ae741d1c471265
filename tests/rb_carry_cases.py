"""Inputs on both sides of the reduction's carry (csrc/gl_rb.hpp).

gl_reduce128_rb, gl_reduce96_small_rb and the small-exponent arm of mul2e_rb
end in t0 + hl EPS, a 65-bit sum whose 65th bit is the carry-out of one
multiply-add: a lane mask in a scalar register pair that selects the + EPS
(gl_reduce128_rb) or is the rare branch's condition (the other two).  Unlike
the rare corrections of tests/rb_cases.py this carry is common (about half of
random products), so what needs building is its *placement*: the exact
boundary (sum == 2^64 - 1 / == 2^64), the extremes, and chosen lanes of a wave.
This module restates the device arithmetic in Python integers (`*_sum`,
`carries`), builds the boundary inputs (`red128_*`, `red96s_*`, `mul2e_side`)
and draws inputs with a wanted carry (`draw`).  tests/test_rb_carry_cases.py
checks the constructions on the CPU, tests/test_gpu_rb_carry.py runs them
through zkgpu_gl_field_selftest_rb_dev.
"""
import rb_cases as rc

P, EPS, M64 = rc.P, rc.EPS, rc.M64
M32 = 0xFFFFFFFF
W = 1 << 64


# ------------------------------------------------------------ device arithmetic
def red128_sum(lo, hi):
    """(t0 + hl EPS, borrow): gl_reduce128_rb's 65-bit sum and whether lo - hh
    borrowed (the rare correction of rb_cases.taken_red128)"""
    hh, hl = hi >> 32, hi & M32
    t0 = (lo - hh) % W
    if lo < hh:
        t0 = (t0 - EPS) % W
    return t0 + hl * EPS, lo < hh


def red128_value(lo, hi):
    """the lazy u64 gl_reduce128_rb returns"""
    s, _ = red128_sum(lo, hi)
    r = s % W + (EPS if s >> 64 else 0)
    assert r < W  # after a carry r <= 2^64 - 2^33: + EPS cannot carry again
    return r


def red96s_sum(lo, hl):
    return lo + (hl & M32) * EPS


def mul2e_sum(e, x):
    """the small-exponent arm of mul2e_rb<e> (0 < e <= ZK_RB_SHIFT_MAX_E)"""
    return ((x << e) % W) + (x >> (64 - e)) * EPS


def sqr_value(x):
    return red128_value(x * x % W, x * x >> 64)


def mul_value(a, b):
    return red128_value(a * b % W, a * b >> 64)


def carries(op, a, b=0, c=0, e=0):
    """does the reduction that produces op's result carry?  (pow7: its last
    product x^3 x^4, on the lazy intermediates the device forms)"""
    if op == rc.RED128:
        return red128_sum(a, b)[0] >> 64 == 1
    if op == rc.MUL:
        return red128_sum(a * b % W, a * b >> 64)[0] >> 64 == 1
    if op == rc.SQR3:
        return carries(rc.MUL, a, a)
    if op == rc.POW7:
        x2 = sqr_value(a)
        return carries(rc.MUL, mul_value(x2, a), sqr_value(x2))
    if op == rc.RED96S:
        return red96s_sum(a, b) >> 64 == 1
    if op == rc.DOTFIN:
        return red128_sum(*rc.dot_words(a, b, c))[0] >> 64 == 1
    if op == rc.MUL2E_RB:
        return mul2e_sum(e, a) >> 64 == 1
    raise ValueError(op)


# ------------------------------------------------------------ boundary inputs
def red128_from(t0, hl, hh=0):
    """(lo, hi) with no borrow whose sum is t0 + hl EPS"""
    lo = t0 + hh
    assert 0 <= t0 and lo <= M64 and hl <= M32 and hh <= M32
    return lo, (hh << 32) | hl


def red128_boundary(rng, carry, hh_max=M32):
    """sum == 2^64 (carry, r = 0) or == 2^64 - 1 (the largest without)"""
    hl = rng.randint(1, M32)
    t0 = W - hl * EPS - (0 if carry else 1)
    return red128_from(t0, hl, rng.randint(0, min(hh_max, M64 - t0)))


def red128_largest():
    """hl = 2^32 - 1 on t0 = 2^64 - 1: the largest sum, 2^64 - 1 + EPS^2"""
    return red128_from(M64, M32)


def red128_hl0(rng, t0=None, hh_max=M32):
    """hl = 0: the multiply-add adds nothing, no carry whatever t0 is"""
    t0 = rng.randint(0, M64) if t0 is None else t0
    return red128_from(t0, 0, rng.randint(0, min(hh_max, M64 - t0)))


def red128_borrow_carry(rng, hh_max=M32):
    """lo < hh (the rare borrow correction) and then a carry, in one element"""
    hh = rng.randint(1, hh_max)
    lo = rng.randint(0, hh - 1)
    t0 = lo - hh + W - EPS            # after the correction; >= 2^64 - 2^33
    hl = rng.randint(-(-(W - t0) // EPS), M32)
    return lo, (hh << 32) | hl


def red96s_boundary(rng, carry):
    hl = rng.randint(1, M32)
    return W - hl * EPS - (0 if carry else 1), hl


def dotfin_from(lo, hi):
    """Dot3 accumulators whose (l2, h) is (lo, hi): A0 = lo, A1 = 0,
    A2 = hi 2^21 (hi < 2^43, so A2 2^43 = hi 2^64 exactly)"""
    assert hi < 1 << 43
    return lo, 0, hi << 21


def mul2e_side(e, rng, carry):
    """x whose sum is the nearest to 2^64 on the wanted side.  lo = x << e is
    a multiple of 2^e and hl EPS (0 < hl < 2^e, EPS odd) is not, so the sum is
    never 2^64 itself: the largest no-carry lo for this hl, or 2^e more."""
    hl = rng.randint(1, (1 << e) - 1)
    lo = ((M64 - hl * EPS) >> e) << e
    if carry:
        lo += 1 << e
    assert 0 <= lo <= M64
    return (hl << (64 - e)) | (lo >> e)


# ------------------------------------------------------------ lanes
def _ordinary(op, rng, e):
    a, b, c = rc.ordinary(rng, 3) if rng.random() < 0.5 else rc.ordinary(rng, 4)[1:]
    if op == rc.RED96S:
        b &= M32
    return a, b, c


def draw(op, rng, carry, e=0):
    """an ordinary lazy input (half of the words in [p, 2^64)) whose reduction
    carries / does not carry; the small shifts carry too rarely to reject for
    (about 2^(e-32)), so their carrying inputs are rb_cases.force_mul2e's"""
    if op == rc.MUL2E_RB and carry:
        return rc.force_mul2e(e, rng), 0, 0
    while True:
        v = _ordinary(op, rng, e)
        if carries(op, *v, e=e) == carry:
            return v


def special(op, rng, carry, k, e=0):
    """the k-th boundary construction of op on the wanted side of the carry,
    as the op's (a, b, c); None where op has none (the products: their
    128-bit value cannot be chosen freely)"""
    hh_max = M32 if op == rc.RED128 else (1 << 11) - 1  # dotfin_from: hi < 2^43
    if op in (rc.RED128, rc.DOTFIN):
        if carry:
            v = [red128_boundary(rng, True, hh_max), red128_largest(), red128_borrow_carry(rng, hh_max)][k % 3]
        else:
            v = [red128_boundary(rng, False, hh_max), red128_hl0(rng, None, hh_max), red128_hl0(rng, M64)][k % 3]
        return v + (0,) if op == rc.RED128 else dotfin_from(*v)
    if op == rc.RED96S:
        if carry:
            return [red96s_boundary(rng, True), (M64, M32)][k % 2] + (0,)
        return [red96s_boundary(rng, False), (rng.randint(0, M64), 0), (M64, 0)][k % 3] + (0,)
    if op == rc.MUL2E_RB:
        return mul2e_side(e, rng, carry), 0, 0
    return None


def wave(op, pattern, rng, e=0, lanes=64):
    """one wave's inputs: the lanes PATTERNS[pattern] names carry, the others
    do not; every third lane of either kind is a boundary construction where
    op has one, the rest are ordinary lazy values"""
    rows = []
    for lane in range(lanes):
        carry = PATTERNS[pattern](lane)
        lone = carry and pattern in ("lane0", "lane63", "middle")
        v = special(op, rng, carry, rng.randrange(6), e) if lane % 3 == 0 or lone else None
        rows.append(v if v is not None else draw(op, rng, carry, e))
    return rows


# which lanes of a 64-lane wave carry
PATTERNS = {
    "all": lambda lane: True,
    "none": lambda lane: False,
    "lane0": lambda lane: lane == 0,
    "lane63": lambda lane: lane == 63,
    "middle": lambda lane: lane == 37,
    "alternating": lambda lane: lane % 2 == 1,
    "lower32": lambda lane: lane < 32,
    "upper32": lambda lane: lane >= 32,
}
