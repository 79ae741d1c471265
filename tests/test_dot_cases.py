"""CPU checks of the dot-product cases (tests/dot_cases.py): the Python model
of Dot3 is right, every builder's compiled program equals its source on the
oracle's evaluators at worst-case and random inputs, the oversized-form split
of the compiler and the fused-chain refill of the kernel printer are really
taken, no DOT of any compiled program the suite knows can wrap an accumulator,
and the worst-case inputs sit where they claim: near the bound."""
import os
import random
import sys

import numpy as np
import pytest

import dot_cases as dc
import rb_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = dc.P


@pytest.fixture(scope="module")
def zkgpu_host():
    import zkgpu
    zkgpu.lib()
    return zkgpu


BUILDERS = {
    "wide_sum_249": lambda: dc.wide_sum(249), "wide_sum_250": lambda: dc.wide_sum(250),
    "wide_sum_251": lambda: dc.wide_sum(251), "wide_sum_500": lambda: dc.wide_sum(500),
    "wide_sum_700": lambda: dc.wide_sum(700), "wide_sum_250_dim1": lambda: dc.wide_sum(250, 1),
    "wide_sum_700_dim1": lambda: dc.wide_sum(700, 1), "chains_800": lambda: dc.chains(800),
    "combine_store_200": lambda: dc.combine_store(200, 200), "combine_store_256": lambda: dc.combine_store(256, 256),
    "temp_terms_90": lambda: dc.temp_terms(90),
}
_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = BUILDERS[name]()
    return _cases[name]


# ---------------------------------------------------------------- the model
def test_pool_is_what_the_search_finds():
    assert dc.search_pool() == (dc.C_TOP0, dc.C_TOP1, dc.C_TOP2, dc.C_JOINT)
    assert min(dc.ratios(dc.C_JOINT)) >= 0.9
    for j, c in enumerate((dc.C_TOP0, dc.C_TOP1, dc.C_TOP2)):
        assert dc.ratios(c)[j] > 0.999
    assert dc.A_MAX < P and dc.A_MAX & dc.M32 == dc.M32 and dc.A_MAX >> 32 == dc.M32 - 1


def test_limbs_recombine():
    rng = random.Random(1)
    for c in [0, 1, P - 1, dc.C_JOINT, dc.A_MAX] + [rng.randrange(P) for _ in range(200)]:
        l = dc.limbs6(c)
        assert l[0] + (l[1] << 22) + (l[2] << 43) == c
        assert (l[3] + (l[4] << 22) + (l[5] << 43)) % P == (c << 32) % P
        assert max(l[0], l[3]) <= dc.LIMB_MAX[0] and max(l[1], l[2], l[4], l[5]) <= dc.LIMB_MAX[1]
        # the vectorised limb sums of the static check agree
        s = dc.limb_sums(np.array([c], np.uint64))
        assert [int(x[0]) for x in s] == [l[j] + l[3 + j] for j in range(3)]


def test_fin_model():
    """fin of random and of extreme accumulators is (A0 + A1 2^22 + A2 2^43)
    mod p, and agrees with rb_cases' DOTFIN reference and branch words."""
    rng = random.Random(2)
    accs = [(0, 0, 0), (dc.M64,) * 3, (dc.M64, 0, 0), (0, dc.M64, 0), (0, 0, dc.M64), (1 << 63,) * 3]
    accs += [tuple(rng.randint(0, dc.M64) for _ in range(3)) for _ in range(300)]
    accs += [rc.force_dotfin(rng) for _ in range(100)]
    for a in accs:
        want = (a[0] + (a[1] << 22) + (a[2] << 43)) % P
        assert dc.fin_words(*a) == want == rc.ref(rc.DOTFIN, *a)
        l2, h = rc.dot_words(*a)
        assert (l2 + (h << 64)) % P == want


def test_dot3_model_sums_terms():
    rng = random.Random(3)
    for n in (1, 7, 250):
        d = dc.Dot3(cst := rng.randrange(P))
        want = cst
        for _ in range(n):
            a, c = rng.choice([dc.A_MAX, dc.M64, rng.randint(0, dc.M64)]), rng.choice([dc.C_JOINT, rng.randrange(P)])
            d.term(a, dc.limbs6(c))
            want += a * c
        assert max(d.acc) < 1 << 63  # the design bound at 250 terms + constant
        assert d.fin() == d.exact() == want % P
        x = d.fin()
        e = dc.Dot3()
        e.lane(x)
        assert e.fin() == x and e.acc[0] < 1 << 32 and e.acc[1] < 1 << 42
    # one term more than 2^64 / TERM_MAX can hold: the registers lose the value
    d = dc.Dot3()
    for _ in range(600):
        d.term(dc.A_MAX, dc.limbs6(dc.C_JOINT))
    assert max(d.acc) > dc.M64 and d.fin() != d.exact()


# ---------------------------------------------------------------- compiled == source
@pytest.mark.parametrize("max_terms", [0, 3, 256])
@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_compiled_equals_source(oracle, zkgpu_host, name, max_terms):
    c = case(name)
    for worst in (True, False):
        inp = dc.Inputs(c, worst, seed=len(name) + max_terms + worst)
        comp = zkgpu_host.zxp_compile(c.prog, inp.chal, inp.pub, inp.evals, max_terms=max_terms)
        want = dc.oracle_eval(oracle, c, inp)
        got = dc.oracle_eval(oracle, c, inp, compiled=comp)
        for k in c.widths:
            assert np.array_equal(want[k], got[k]), "section %d differs (worst=%s)" % (k, worst)
        assert not np.array_equal(want[dc.SEC_OUT], inp.S[dc.SEC_OUT])  # it wrote something
        if name.startswith("wide_sum"):
            K, dim = len(c.prog.instr) // 2, 1 if name.endswith("dim1") else 3
            rows = [0, 1, 255, 256, 300, inp.dom - 1]
            ref = dc.wide_sum_rows(K, dim, inp, rows)
            for i, r in zip(rows, ref):
                assert [int(x) for x in want[dc.SEC_OUT][i, :dim]] == r[:dim], (i, worst)


# ---------------------------------------------------------------- the split path
@pytest.mark.parametrize("name", ["wide_sum_500", "wide_sum_700", "combine_store_200", "combine_store_256"])
def test_split_path_taken(zkgpu_host, name):
    """At max_terms = 256 the source builds a form of more than DOT_HARD_CAP
    terms (counted here on the source program); emit_dot splits it, and no
    DOT of the compiled program exceeds the cap, constant included."""
    c = case(name)
    biggest = dc.largest_form(c.prog, 256)
    assert biggest + 1 > dc.DOT_CAP, biggest
    inp = dc.Inputs(c, True, seed=5)
    comp = zkgpu_host.zxp_compile(c.prog, inp.chal, inp.pub, inp.evals, max_terms=256)
    counts = [b for _k, _a, b, _dim in dc.dot_instrs(comp)]
    print("%s: largest source form %d terms, compiled DOTs %s" % (name, biggest, sorted(counts)[-4:]))
    assert max(counts) <= dc.DOT_CAP
    # the split produced a full piece (cap - 1 terms, no constant) fed into a later DOT
    assert dc.DOT_CAP - 1 in counts and len(counts) >= 2


def test_largest_form_counts(zkgpu_host):
    """largest_form agrees with the compiler where the compiler's own DOTs
    show the form: below the cap a stored form is one DOT of that size."""
    for K1, K2 in ((100, 100), (60, 180)):
        c = dc.combine_store(K1, K2)
        inp = dc.Inputs(c, True, seed=6)
        comp = zkgpu_host.zxp_compile(c.prog, inp.chal, inp.pub, inp.evals, max_terms=256)
        assert [b for _k, _a, b, _d in dc.dot_instrs(comp)] == [K1 + K2] == [dc.largest_form(c.prog, 256)]


# ---------------------------------------------------------------- static headroom
def _known_programs(zkgpu_host):
    from zkgpu.synthetic import SyntheticStark
    rng = np.random.default_rng(9)
    for name in sorted(BUILDERS):
        c = case(name)
        for worst in (True, False):
            inp = dc.Inputs(c, worst, seed=7)
            for mt in (0, 3, 256):
                yield "%s/%d/%d" % (name, worst, mt), c.prog, inp.chal, inp.pub, inp.evals, mt
    for t in (6, 30):
        inst = SyntheticStark(n_bits=5, t=t, m=2, n_free=5 if t == 6 else 8, n_lookups=2, n_queries=4)
        for name, prog in inst.programs.items():
            if not prog.instr:
                continue
            for worst in (True, False):
                draw = dc.pool_values if worst else dc.rand_canon
                for mt in (0, 3, 256):
                    yield ("synthetic t=%d %s/%d/%d" % (t, name, worst, mt), prog, draw(rng, (8, 3)),
                           draw(rng, inst.n_publics), draw(rng, (len(inst.evmap), 3)), mt)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import jit_prebuild as jp
    ch, pub, ev = jp.consts()
    for scale, name in ((1.0, "step52ns"), (1.0, "step3prev"), (0.25, "step42ns")):
        prog = jp.program(scale, name)
        yield "zkevm-shaped %s" % name, prog, ch, pub, ev, 0
        yield ("zkevm-shaped %s/pool/256" % name, prog, dc.pool_values(rng, ch.shape), dc.pool_values(rng, pub.shape),
               dc.pool_values(rng, ev.shape), 256)


def _assert_headroom(zkgpu_host, programs):
    top = (0, 0, "")
    for label, prog, ch, pub, ev, mt in programs:
        comp = zkgpu_host.zxp_compile(prog, ch, pub, ev, max_terms=mt)
        counts = [b for _k, _a, b, _d in dc.dot_instrs(comp)]
        acc, nt = dc.static_headroom(comp)
        top = max(top, (acc, nt, label))
        assert acc < 1 << 64, "%s: a %d-term DOT reaches %.3f x 2^64" % (label, nt, acc / 2.0**64)
        assert not counts or max(counts) <= dc.DOT_CAP, "%s: a DOT of %d terms" % (label, max(counts))
    print("largest accumulator: %.4f x 2^63 (%d terms, %s)" % (top[0] / 2.0**63, top[1], top[2]))
    return top


def test_static_headroom(zkgpu_host):
    """Every source word at 2^64 - 1 against each program's own coefficient
    limbs: no accumulator of any DOT reaches 2^64 (the true wrap limit; the
    design bound is 2^63), and no DOT exceeds the cap."""
    top = _assert_headroom(zkgpu_host, _known_programs(zkgpu_host))
    assert top[0] > 0.85 * (dc.DOT_CAP - 1) * dc.TERM_MAX[0]  # the builders do load the accumulators


REF = "/root/reference/src/starkpil/starkRecursive1/chelpers"


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference sources not present")
@pytest.mark.parametrize("which", ["step52ns", "step42ns"])
def test_static_headroom_reference_step_code(zkgpu_host, which):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import chelpers_zxp as cz
    from zkgpu.synthetic import SEC_CM1_2NS, SEC_CM3_2NS, SEC_CM4_2NS
    secs = {18: (SEC_CM1_2NS, 11010048), 39: (SEC_CM3_2NS, 29884416), 21: (SEC_CM4_2NS, 70778880)}
    prog, _ = cz.translate_file(os.path.join(REF, "recursive1.chelpers.%s.cpp" % which), "%s_first" % which, secs, 1)
    opn = np.array(prog.opnd, np.int64).reshape(-1, 4)
    n_ev = int(opn[opn[:, 0] == 8][:, 1].max()) + 1 if (opn[:, 0] == 8).any() else 1
    n_pub = int(opn[opn[:, 0] == 6][:, 1].max()) + 1 if (opn[:, 0] == 6).any() else 1
    rng = np.random.default_rng(10)
    _assert_headroom(zkgpu_host, [
        ("recursive1 %s" % which, prog, dc.rand_canon(rng, (8, 3)), dc.rand_canon(rng, n_pub),
         dc.rand_canon(rng, (n_ev, 3)), 0),
        ("recursive1 %s/pool/256" % which, prog, dc.pool_values(rng, (8, 3)), dc.pool_values(rng, n_pub),
         dc.pool_values(rng, (n_ev, 3)), 256)])


# ---------------------------------------------------------------- the worst case is near the bound
def test_worst_case_is_near_the_bound(zkgpu_host):
    """A condition on the inputs: on an all-A_MAX row the longest DOT of
    wide_sum(250) holds at least 0.85 of nterms x the per-term maximum in each
    accumulator of each component (so the GPU cases test what they claim)."""
    c = case("wide_sum_250")
    inp = dc.Inputs(c, True, seed=11)
    comp = zkgpu_host.zxp_compile(c.prog, inp.chal, inp.pub, inp.evals, max_terms=256)
    k, _a, nt, dim = max(dc.dot_instrs(comp), key=lambda d: d[2])
    assert nt == dc.DOT_CAP - 1 and dim == 3
    row = 7  # rows 0..255 (and their +1 neighbours) are all A_MAX

    def src(o, _comp):
        assert o[0] == dc.COL and o[1] == dc.SEC_IN
        return int(inp.S[dc.SEC_IN][(row + np.int32(o[3])) % inp.dom, o[2]])

    for j, (acc, val) in enumerate(dc.accumulators(comp, k, src)):
        share = [acc[w] / (nt * dc.TERM_MAX[w]) for w in range(3)]
        print("component %d: accumulators at %s of %d terms' maximum, %s x 2^63" % (
            j, ["%.3f" % s for s in share], nt, ["%.3f" % (a / 2.0**63) for a in acc]))
        assert min(share) >= 0.85
        assert max(acc) < 1 << 63
        want = sum(int(t["coef"][j]) * src(tuple(int(x) for x in comp["opnd"][int(t["src"])]), 0)
                   for t in comp["term"][_a:_a + nt])
        assert val == want % P
    # random inputs: about a quarter of that
    rnd = dc.Inputs(c, False, seed=11)
    compr = zkgpu_host.zxp_compile(c.prog, rnd.chal, rnd.pub, rnd.evals, max_terms=256)
    acc, _ = dc.accumulators(compr, k, lambda o, _c: int(rnd.S[dc.SEC_IN][(600 + np.int32(o[3])) % rnd.dom, o[2]]))[0]
    assert max(acc[w] / (nt * dc.TERM_MAX[w]) for w in range(3)) < 0.4


def test_input_layout():
    c = case("wide_sum_250")
    a = dc.Inputs(c, True, seed=1).S[dc.SEC_IN]
    assert (a[:256] == dc.A_MAX).all() and (a < P).all()
    for w0 in range(256, 512, 64):
        full = [(a[w0 + l] == dc.A_MAX).all() for l in range(64)]
        assert full[0] and full[63] and sum(full) == 3
    assert not (a[512:] == dc.A_MAX).all(axis=1).any()
    assert not (dc.Inputs(c, False, seed=1).S[dc.SEC_IN] == dc.A_MAX).any()


# ---------------------------------------------------------------- kernel text
def _source(zkgpu_host, c, inp, rtc_check):
    return zkgpu_host.zxp_jit_source(c.prog, inp.chal, inp.pub, inp.evals, rtc_check=rtc_check)


@pytest.mark.parametrize("name", ["chains_800", "wide_sum_500", "temp_terms_90"])
def test_kernel_text_takes_the_intended_path(zkgpu_host, name):
    """The kernel printed for each builder (compiled by hiprtc for gfx950, no
    GPU needed): chains as fused loops with a reduce-and-refill block,
    wide_sum(500) with looped DOTs, temp_terms with neither; the text does not
    depend on the challenges and evals."""
    c = case(name)
    worst, rnd = dc.Inputs(c, True, seed=12), dc.Inputs(c, False, seed=13)
    src = _source(zkgpu_host, c, worst, True)
    assert src == _source(zkgpu_host, c, rnd, False)
    if name.startswith("chains"):
        assert src.count("for (int q_") >= 4  # one loop per group of chains sharing columns
        assert ".lane(x0_)" in src
    else:
        assert "for (int q_" not in src and ".lane(x0_)" not in src
    assert ("dot_cols<3>(" in src) == name.startswith("wide_sum")
    if name.startswith("temp_terms"):
        assert "dot_cols<" not in src


def test_fused_chains_reduce_in_time(zkgpu_host):
    """The fused chains' own count (emit_fused, csrc/zxp_jit_source.cpp), read off the
    printed kernel: between two reductions no chain accumulator takes more
    than the cap's terms (the re-seeding lane and the constant included), for
    chains(800) and for the zkEVM-shaped FRI polynomial."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import jit_prebuild as jp
    c = case("chains_800")
    inp = dc.Inputs(c, True, seed=12)
    for label, src in (("chains(800)", _source(zkgpu_host, c, inp, False)),
                       ("zkevm-shaped step52ns", zkgpu_host.zxp_jit_source(jp.program(1.0, "step52ns"), *jp.consts()))):
        fill = dc.fused_fill(src)
        print("%s: at most %d terms between two reductions" % (label, fill))
        assert 128 <= fill and fill + 1 <= dc.DOT_CAP
    # chains(800): groups of 200 columns, so a chain is reduced before every group but its first
    assert dc.fused_fill(_source(zkgpu_host, c, inp, False)) == 201
