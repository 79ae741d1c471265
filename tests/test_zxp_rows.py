"""tests/zxp_rows.py, the checker of the prover's probe, against the oracle:
eval_rows on sampled rows == oc_zxp_eval on the whole domain for all five
programs of both instances (wrap rows included), and check_probe finds a
flipped bit where it was flipped.  CPU only."""
import copy

import numpy as np
import pytest

import zxp_rows as zr
from test_oracle_rows import sample_rows


def _inst(kind):
    import bench
    return bench.stark_instance(10, 1, 100, 16, kind)


def _rows(inst, seed=5):
    rng = np.random.default_rng(seed)
    return (sample_rows(1 << inst.n_bits, rng, n_random=32)[0],
            sample_rows(1 << inst.n_bits_ext, rng, n_random=32)[0])


@pytest.fixture(scope="module")
def probes(oracle):
    """{kind: (inst, publics, records)} of one oracle proof each (shared, never modified)"""
    from oracle.stark_prover import OracleStark
    out = {}
    for kind in (False, "zkevm"):
        inst = _inst(kind)
        o = OracleStark(inst)
        o.witness()
        rn, re_ = _rows(inst)
        recs, proof = zr.oracle_probe(o, rn, re_)
        out[kind] = (inst, o.publics.copy(), recs, proof)
    return out


def _edit(recs, point, after, sec):
    """a deep copy of the records and the index of one of them"""
    recs = [(p, a, s, r.copy(), v.copy()) for p, a, s, r, v in recs]
    k = [i for i, (p, a, s, _, _) in enumerate(recs) if (p, a, s) == (point, after, sec)]
    assert len(k) == 1
    return recs, k[0]


@pytest.mark.parametrize("kind", [False, "zkevm"], ids=["config4", "zkevm_shaped"])
def test_oracle_probe_checks_clean(probes, kind):
    """eval_rows == oc_zxp_eval on every stored column of every program point;
    no point's comparison is empty or all zero"""
    inst, publics, recs, _ = probes[kind]
    stats = {}
    assert zr.check_probe(inst, recs, publics, stats) == []
    want = {pt for pt, name in zr.PROGRAM_POINTS.items() if inst.programs.get(name) and inst.programs[name].instr}
    assert set(stats) == want and len(want) == 5
    for pt, st in stats.items():
        assert st["cols"] >= 1 and st["rows"] >= 32 and st["nonzero"], (zr.POINT_NAMES[pt], st)
    # the rows of the (i + s) mod dom wrap are among those compared
    by = zr.split_probe(recs)
    for pt in want:
        dom = 1 << (inst.n_bits_ext if pt >= zr.STEP42NS else inst.n_bits)
        for sec, (rows, _) in by[pt]["after"].items():
            assert {0, dom - 1} <= set(rows.tolist())


def test_oracle_probe_leaves_the_proof_alone(probes, oracle):
    from oracle.stark_prover import OracleStark
    inst, _, _, proof = probes[False]
    o = OracleStark(inst)
    o.witness()
    assert o.prove() == proof


def test_flipped_quotient_value_is_located(probes):
    inst, publics, recs, _ = probes["zkevm"]
    recs, k = _edit(recs, zr.STEP42NS, 1, 10)
    rows, vals = recs[k][3], recs[k][4]
    i = rows.size // 2
    vals[i, 1] ^= np.uint64(1 << 17)
    assert zr.check_probe(inst, recs, publics) == [(zr.STEP42NS, 10, int(rows[i]), 1)]


def test_flipped_shifted_read_is_noticed(probes):
    """a cm1 value step42ns reads only through a shifted access (a row of the
    before-record that is not itself sampled)"""
    inst, publics, recs, _ = probes["zkevm"]
    _, shifts_ok, shifts = zr.program_sections(inst.programs["step42ns"])
    assert any(s != 0 for s in shifts[zr.SEC_CM1_2NS])
    ins, opn = inst.programs["step42ns"].arrays()
    col = next(int(o[2]) for o in opn if o[0] in (zr.COL, zr.COL3) and o[1] == zr.SEC_CM1_2NS and zr._shift(o[3]) != 0)
    recs, k = _edit(recs, zr.STEP42NS, 0, zr.SEC_CM1_2NS)
    rows, vals = recs[k][3], recs[k][4]
    sampled = set(_rows(inst)[1].tolist())
    i = next(j for j, r in enumerate(rows.tolist()) if r not in sampled)
    vals[i, col] ^= np.uint64(1)
    bad = zr.check_probe(inst, recs, publics)
    assert bad and all(b[:2] == (zr.STEP42NS, 10) for b in bad)


def test_flipped_challenge_is_noticed(probes):
    inst, publics, recs, _ = probes[False]
    recs, k = _edit(recs, zr.STEP2, 0, zr.SCALARS)
    recs[k][4][0, 1] ^= np.uint64(1 << 40)
    bad = zr.check_probe(inst, recs, publics)
    assert bad and all(b[0] == zr.STEP2 for b in bad)


def test_shifted_read_of_own_store_raises():
    from zkgpu import synthetic as sy
    p = sy.Program(0)
    src = p.o(sy.COL, sy.SEC_CM1_N, 0, 0)
    p.op(sy.COPY, p.o(sy.COL, sy.SEC_TMP_N, 0, 0), src)
    p.op(sy.ADD, p.o(sy.COL, sy.SEC_TMP_N, 1, 0), p.o(sy.COL, sy.SEC_TMP_N, 0, 1), src)
    rows = np.arange(4, dtype=np.uint64)
    before = {sy.SEC_CM1_N: (rows, np.ones((4, 1), np.uint64)), sy.SEC_TMP_N: (rows, np.zeros((4, 2), np.uint64))}
    with pytest.raises(ValueError, match="shifted read"):
        zr.eval_rows(p, 2, False, 1, before, np.zeros(24, np.uint64), [])
    # the same read at the store's own shift sees the stored value
    q = sy.Program(0)
    src = q.o(sy.COL, sy.SEC_CM1_N, 0, 0)
    d = q.o(sy.COL, sy.SEC_TMP_N, 0, 0)
    q.op(sy.COPY, d, src)
    q.op(sy.ADD, q.o(sy.COL, sy.SEC_TMP_N, 1, 0), d, src)
    out = zr.eval_rows(q, 2, False, 1, before, np.zeros(24, np.uint64), [])
    assert out[(sy.SEC_TMP_N, 1)][1].tolist() == [2, 2, 2, 2]
