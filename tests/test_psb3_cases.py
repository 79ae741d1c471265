"""CPU checks of the power-block form of the Poseidon partial rounds
(tools/gen_poseidon_sparse.py derive_pow_blocks / perm_pow_blocks) and of the
constructed inputs of tests/psb3_cases.py, in Python integers."""
import random

import pytest

import psb3_cases as pc

gen, P = pc.gen, pc.P


def _check_acc(lo, hi):
    assert lo <= pc.ACC_MAX and hi <= pc.ACC_MAX


@pytest.mark.parametrize("name", sorted(pc.SCHEDULES))
def test_block_model_equals_textbook(name):
    sched, ktab = pc.SCHEDULES[name], pc.KTAB[name]
    states = pc.edge_states() + pc.random_states(24, 31)
    states += [pc.state_with_lane0_after_full4(t, 7 + t % 5) for t in (0, P - 1)]
    for st in states:
        assert gen.perm_pow_blocks(st, pc.RC, pc.PRE, sched, ktab, _check_acc) == gen.perm_textbook(st, pc.RC)


@pytest.mark.parametrize("name", sorted(pc.SCHEDULES))
def test_blocks_take_lazy_lanes(name):
    """a block's dot products are integer sums: lanes >= p (lazy words) give the same residues,
    and the accumulators stay in range for ANY u64 lanes"""
    rng = random.Random(5)
    sched, ktab = pc.SCHEDULES[name], pc.KTAB[name]
    for n, words in zip(sched, ktab):
        s = [rng.randrange(P) for _ in range(12)]
        lazy = [v + P if v + P <= pc.M64 and rng.random() < 0.5 else v for v in s]
        assert gen.pow_block_eval(lazy, words, n, _check_acc) == gen.pow_block_eval(s, words, n, _check_acc)
        gen.pow_block_eval([pc.M64] * 12, words, n, _check_acc)


def test_accumulator_bound():
    """from the integer row sums alone: seed + (2^32 - 1) * (coefficient sum) for every dot
    product of every block length, S-box terms included"""
    for n in (1, 2, 3):
        worst = gen.pow_acc_bound(n)
        assert worst < 1 << 64
        assert worst <= pc.ACC_MAX
        for _, _, coef in gen.pow_block_rows(n):
            assert all(0 <= c < 1 << 21 for c in coef)
    P1, P2, P3 = gen.pow_mats()
    M = gen.mds()
    assert P1 == M
    # entrywise below the plain powers of M
    M2 = [[sum(M[i][t] * M[t][j] for t in range(12)) for j in range(12)] for i in range(12)]
    M3 = [[sum(M2[i][t] * M[t][j] for t in range(12)) for j in range(12)] for i in range(12)]
    assert all(P2[i][j] <= M2[i][j] and P3[i][j] <= M3[i][j] for i in range(12) for j in range(12))
    assert max(max(r) for r in M3) < 1 << 21


def test_lane0_states():
    for t in (0, P - 1):
        st = pc.state_with_lane0_after_full4(t, 3)
        assert all(0 <= v < P for v in st)
        assert pc.after_full4(st)[0] == t


def test_fin_cases():
    rng = random.Random(58)
    seen = set()
    for mc, ec in pc.FIN_COMBOS:
        for hmax in (pc.ACC_MAX, pc.WIDE):
            if mc and ec and hmax == pc.ACC_MAX:
                continue
            for _ in range(8):
                L, H = pc.force_fin(rng, mc, ec, hmax)
                assert 0 <= L <= (hmax if hmax == pc.ACC_MAX else pc.M64) and 0 <= H <= hmax
                # the conditions restated from Dot2::fin's text
                mid = (L >> 32) + (H & pc.W32)
                assert (mid > pc.W32) == mc == pc.fin_mid_carry(L, H)
                lo = ((mid & pc.W32) << 32) | (L & pc.W32)
                h = (H >> 32) + (1 if mc else 0)
                assert (lo + h * pc.EPS >= 1 << 64) == ec == pc.fin_eps_carry(L, H)
                assert pc.fin_model(L, H) % P == pc.fin_ref(L, H)
            seen.add((mc, ec, hmax == pc.ACC_MAX))
    assert len(seen) == 7
    names = set()
    for name, L, H in pc.fin_boundary_cases():
        assert 0 <= L <= pc.M64 and 0 <= H < 1 << 63
        lo, h, _ = pc.fin_words(L, H)
        if name == "eps_at":
            assert lo + h * pc.EPS == 1 << 64 and pc.fin_eps_carry(L, H) and pc.fin_model(L, H) == pc.EPS
        if name == "eps_below":
            assert lo + h * pc.EPS == pc.M64 and not pc.fin_eps_carry(L, H)
        assert pc.fin_model(L, H) % P == pc.fin_ref(L, H)
        names.add(name)
    assert names == {"zero", "acc_max", "l_max", "h_only", "wide", "eps_at", "eps_below"}
    # inside the kernel range a mid carry excludes the EPS carry
    for _ in range(2000):
        L, H = rng.randint(0, pc.ACC_MAX), rng.randint(0, pc.ACC_MAX)
        assert not (pc.fin_mid_carry(L, H) and pc.fin_eps_carry(L, H))
        assert pc.fin_model(L, H) % P == pc.fin_ref(L, H)


def test_committed_header_is_the_generators():
    """csrc/poseidon_gl_sparse.h carries the device schedule's seeds as the generator derives them"""
    import os
    import re
    text = open(os.path.join(pc._ROOT, "zkevm-prover_amd", "csrc", "poseidon_gl_sparse.h")).read()
    m = re.search(r"ZKGPU_PSB3_K\[(\d+)\] = \{(.*?)\};", text, re.S)
    vals = [int(t, 16) for t in re.findall(r"0x([0-9a-f]{8})u", m.group(2))]
    ktab = pc.KTAB[gen.POW_SCHEDULE]
    assert vals == [w for t in ktab[:-1] for w in t] and len(vals) == int(m.group(1))
    assert "#define ZKGPU_PSB3_NBLOCKS %d" % (len(ktab) - 1) in text


def test_benchmark_variant_header_is_the_generators():
    """tools/poseidon_bench_alt.h: the 6x3+2x2 schedule's seeds of the isolated benchmark's variant"""
    import os
    import re
    text = open(os.path.join(pc._ROOT, "tools", "poseidon_bench_alt.h")).read()
    sched, ktab = pc.SCHEDULES["6x3+2x2"], pc.KTAB["6x3+2x2"]
    for name, n in (("PSB_ALT_K3", 3), ("PSB_ALT_K2", 2)):
        m = re.search(name + r"\[(\d+)\] = \{(.*?)\};", text, re.S)
        vals = [int(t, 16) for t in re.findall(r"0x([0-9a-f]{8})u", m.group(2))]
        assert vals == [w for nn, t in zip(sched, ktab) if nn == n for w in t] and len(vals) == int(m.group(1))
