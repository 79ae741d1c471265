"""CPU checks of the carry placements (tests/rb_carry_cases.py): every
constructed input meets the condition it was built for, on the restated device
arithmetic, and that restatement agrees with the field."""
import random

import pytest

import rb_carry_cases as cc
import rb_cases as rc

W, M64, M32, EPS, P = cc.W, cc.M64, cc.M32, cc.EPS, cc.P


def test_red128_boundary_sums():
    rng = random.Random(1)
    for _ in range(300):
        lo, hi = cc.red128_boundary(rng, False)
        assert cc.red128_sum(lo, hi) == (W - 1, False) and not cc.carries(rc.RED128, lo, hi)
        lo, hi = cc.red128_boundary(rng, True)
        assert cc.red128_sum(lo, hi) == (W, False) and cc.carries(rc.RED128, lo, hi)
        assert cc.red128_value(lo, hi) == EPS  # r = 0, then + EPS


def test_red128_hl0_never_carries():
    rng = random.Random(2)
    for t0 in [None] * 100 + [0, M64]:
        lo, hi = cc.red128_hl0(rng, t0)
        s, borrow = cc.red128_sum(lo, hi)
        assert hi & M32 == 0 and not borrow and s < W and (t0 is None or s == t0)


def test_red128_largest_sum():
    lo, hi = cc.red128_largest()
    s, borrow = cc.red128_sum(lo, hi)
    assert (lo, hi) == (M64, M32) and not borrow and s == M64 + M32 * EPS and s < 1 << 65
    # after the carry r = s - 2^64 <= 2^64 - 2^33, so r + EPS stays a u64
    assert s - W == W - (1 << 33) and cc.red128_value(lo, hi) == s - W + EPS


def test_red128_borrow_and_carry_in_one_element():
    rng = random.Random(3)
    for _ in range(300):
        lo, hi = cc.red128_borrow_carry(rng)
        s, borrow = cc.red128_sum(lo, hi)
        assert lo < hi >> 32 and rc.taken_red128(lo, hi) and borrow and s >> 64 == 1


def test_red96s_boundary_sums():
    rng = random.Random(4)
    for _ in range(300):
        lo, hl = cc.red96s_boundary(rng, False)
        assert cc.red96s_sum(lo, hl) == W - 1 and not rc.taken_red96s(lo, hl)
        lo, hl = cc.red96s_boundary(rng, True)
        assert cc.red96s_sum(lo, hl) == W and rc.taken_red96s(lo, hl)
    assert cc.red96s_sum(M64, M32) == M64 + M32 * EPS and cc.red96s_sum(M64, 0) == M64


@pytest.mark.parametrize("e", [1, 20])
def test_mul2e_sides(e):
    rng = random.Random(e)
    for _ in range(300):
        x0, x1 = cc.mul2e_side(e, rng, False), cc.mul2e_side(e, rng, True)
        s0, s1 = cc.mul2e_sum(e, x0), cc.mul2e_sum(e, x1)
        # the nearest sums to 2^64 that x << e (a multiple of 2^e) can reach
        assert 0 <= x0 <= M64 and W - (1 << e) <= s0 < W and not rc.taken_mul2e(e, x0)
        assert 0 <= x1 <= M64 and W <= s1 < W + (1 << e) and rc.taken_mul2e(e, x1)


def test_dotfin_from_gives_the_words():
    rng = random.Random(5)
    for _ in range(200):
        lo, hi = cc.red128_boundary(rng, rng.random() < 0.5, (1 << 11) - 1)
        assert rc.dot_words(*cc.dotfin_from(lo, hi)) == (lo, hi)
    lo, hi = cc.red128_borrow_carry(rng, (1 << 11) - 1)
    assert rc.taken_dotfin(*cc.dotfin_from(lo, hi))


OPS = [(rc.MUL, 0), (rc.RED128, 0), (rc.RED96S, 0), (rc.DOTFIN, 0), (rc.MUL2E_RB, 1), (rc.MUL2E_RB, 20), (rc.POW7, 0),
       (rc.SQR3, 0)]


@pytest.mark.parametrize("op,e", OPS)
def test_specials_are_on_their_side(op, e):
    rng = random.Random(10 * op + e)
    for k in range(12):
        for carry in (False, True):
            v = cc.special(op, rng, carry, k, e)
            assert (v is None) == (op in (rc.MUL, rc.POW7, rc.SQR3))
            if v is not None:
                assert all(0 <= w <= M64 for w in v) and cc.carries(op, *v, e=e) == carry


@pytest.mark.parametrize("op,e", OPS)
@pytest.mark.parametrize("pattern", sorted(cc.PATTERNS))
def test_wave_patterns(op, e, pattern):
    rows = cc.wave(op, pattern, random.Random(pattern + str(op) + str(e)), e)
    assert len(rows) == 64
    for lane, v in enumerate(rows):
        assert all(0 <= w <= M64 for w in v)
        assert cc.carries(op, *v, e=e) == cc.PATTERNS[pattern](lane), (lane, v)
    if op in (rc.MUL, rc.POW7, rc.SQR3):
        # the products' operands are free: a good share of lazy words in
        # [p, 2^64) (a reduction's own lo >= p leaves no room for a carry-free hl)
        assert sum(v[0] >= P for v in rows) >= 8


def test_model_matches_the_field():
    rng = random.Random(6)
    for _ in range(300):
        lo, hi = rng.randint(0, M64), rng.randint(0, M64)
        assert cc.red128_value(lo, hi) % P == rc.ref(rc.RED128, lo, hi)
        a, b = rc.ordinary(rng, 2)
        assert cc.mul_value(a, b) % P == a * b % P and cc.sqr_value(b) % P == b * b % P
    for lo, hi in [cc.red128_largest(), cc.red128_boundary(rng, True), cc.red128_borrow_carry(rng)]:
        assert cc.red128_value(lo, hi) % P == rc.ref(rc.RED128, lo, hi)
