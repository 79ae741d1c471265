"""The reduction's carry as a lane mask, on the GPU vs big integers.

csrc/gl_rb.hpp takes the carry of t0 + hl EPS from the multiply-add's
carry-out: a lane mask in a scalar register pair.  So the lane pattern is the
thing under test: every helper that ends in that sum runs through
zkgpu_gl_field_selftest_rb_dev on waves whose carrying lanes are all, none,
lane 0, lane 63, one middle lane, alternating, the lower 32 and the upper 32
(tests/rb_carry_cases.py, checked on the CPU by test_rb_carry_cases.py); the
other lanes hold ordinary lazy values that do not carry, and a third of the
lanes sit on the boundary (sum == 2^64 - 1 / == 2^64, hl = 0, the largest
sum, borrow and carry in one element).  Once on 4096 elements, once with the
last wave partial.  Then the permutation on states of edge words against the
oracle.  Reference semantics: the Goldilocks field ops of starks.cpp:53 and
PoseidonGoldilocks::hash_full_result.
"""
import functools
import random

import numpy as np
import pytest

import rb_carry_cases as cc
import rb_cases as rc

pytestmark = pytest.mark.gpu

N = 4096
OPS = {
    "mul": (rc.MUL, 0),
    "reduce128": (rc.RED128, 0),
    "reduce96_small": (rc.RED96S, 0),
    "dot3_fin": (rc.DOTFIN, 0),
    "mul2e_rb_1": (rc.MUL2E_RB, 1),
    "mul2e_rb_20": (rc.MUL2E_RB, 20),
    "pow7": (rc.POW7, 0),
    "sqr3": (rc.SQR3, 0),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(rows, expected, wave patterns) of one op: 64 waves cycling through
    the eight patterns, built once and shared by both lengths"""
    op, e = OPS[name]
    rng = random.Random("carry " + name)
    pats = [sorted(cc.PATTERNS)[w % len(cc.PATTERNS)] for w in range(N // 64)]
    rows = [v for p in pats for v in cc.wave(op, p, rng, e)]
    exp = [rc.ref(op, *v, e=e) for v in rows]
    return rows, exp, pats


@pytest.mark.parametrize("n", [N, N - 27], ids=["full", "partial_last_wave"])
@pytest.mark.parametrize("name", sorted(OPS))
def test_carry_lane_patterns(zkgpu, name, n):
    import torch
    op, e = OPS[name]
    rows, exp, pats = _case(name)
    for w in (0, len(pats) - 1):  # spot-check the placement (all of it: test_rb_carry_cases.py)
        for lane in (0, 31, 32, 63):
            assert cc.carries(op, *rows[64 * w + lane], e=e) == cc.PATTERNS[pats[w]](lane)
    a, b, c = (zkgpu.to_device(np.array(col[:n], dtype=np.uint64)) for col in zip(*rows))
    out = torch.zeros(n, dtype=torch.int64, device="cuda:0")
    zkgpu.field_selftest_rb_dev(out, a, b, c, n, op, e)
    torch.cuda.synchronize()
    got = zkgpu.from_device(out)
    bad = [i for i in range(n) if int(got[i]) != exp[i]]
    assert not bad, [(i, pats[i // 64], i % 64, [hex(v) for v in rows[i]], hex(int(got[i])), hex(exp[i]))
                     for i in bad[:5]]


def test_permutation_edge_words(oracle, zkgpu):
    """256 states whose lanes are drawn from the edge words, full and 4-lane
    output, against the oracle's permutation (of the canonical words: the
    device takes lazy inputs)"""
    import torch
    P = rc.P
    words = np.array([0, 1, P - 1, P, rc.M64, 2**32 - 1, 2**32], dtype=np.uint64)
    rng = np.random.default_rng(950)
    n = 256
    x = words[rng.integers(0, len(words), size=(n, 12))]
    for k, w in enumerate(words):  # and each word in every lane of a state
        x[k] = w
    din = zkgpu.to_device(x)
    full = torch.zeros((n, 12), dtype=torch.int64, device="cuda:0")
    four = torch.zeros((n, 4), dtype=torch.int64, device="cuda:0")
    zkgpu.poseidon_batch_dev(full, din, n, True)
    zkgpu.poseidon_batch_dev(four, din, n, False)
    torch.cuda.synchronize()
    full, four = zkgpu.from_device(full), zkgpu.from_device(four)
    exp = np.stack([oracle.poseidon_full(x[i] % np.uint64(P)) for i in range(n)])
    assert np.array_equal(full, exp)
    assert np.array_equal(four, exp[:, :4])
