"""The SyntheticStark connection check (zkgpu/synthetic.py n_conns, conn_k) on
the CPU: the default instance is unchanged by the option, the construction is
a clean connection by the pure-Python reference (tests/conn_cases.py), the
oracle proves it and the verifier replays the proof, one altered cell is two
broken links and an open product in the audit's restatement
(tests/audit_cases.py), and the starkinfo lists it under ciCtx."""
import numpy as np
import pytest

import audit_cases as ac
import conn_cases as cc

P = cc.P


def _columns(inst, o, trace, k=0):
    cn = inst.conns[k]
    return (np.ascontiguousarray(trace[:, cn["cols"]].T), np.ascontiguousarray(o.S[4][:, cn["S"]].T), cn["ks"])


def test_default_instance_is_unchanged_by_n_conns():
    from zkgpu import synthetic as sy
    for kw in (dict(), dict(n_bits=8, t=2, m=1, n_perms=1), dict(n_bits=8, n_lookups=0)):
        x, y = sy.SyntheticStark(**kw), sy.SyntheticStark(n_conns=0, conn_k=5, **kw)
        assert x.info() == y.info() and x.conns == []
        for name in x.programs:
            for u, v in zip(x.programs[name].arrays(), y.programs[name].arrays()):
                assert np.array_equal(u, v), name


def test_layout():
    from zkgpu import synthetic as sy
    base = sy.SyntheticStark(n_bits=8, n_perms=1)
    inst = sy.SyntheticStark(n_bits=8, n_perms=1, n_conns=2, conn_k=2)
    assert (inst.n_cm1, inst.n_const, inst.n_cm3, inst.n_tmp) == \
        (base.n_cm1 + 4, base.n_const + 4, base.n_cm3 + 6, base.n_tmp + 12)
    assert inst.z_ctx[:len(base.z_ctx)] == base.z_ctx  # the connections' products come last
    assert inst.z_ctx[len(base.z_ctx):] == [(cn["num"], cn["den"], cn["z"]) for cn in inst.conns]
    assert inst.conns[0]["cols"] == [base.n_cm1, base.n_cm1 + 1] and inst.conns[1]["S"] == [base.n_const + 2,
                                                                                            base.n_const + 3]
    assert [c for c in inst.random_cm1_cols() if c >= base.n_cm1] == [cn["cols"][0] for cn in inst.conns]
    for cn in inst.conns:
        assert sum(r for _, r in inst.conn_wiring(cn)) % (1 << 8) == 0  # the rotations close the cycle
        assert cn["ks"] == cc.default_ks(2)
    with pytest.raises(AssertionError):
        sy.SyntheticStark(n_bits=8, n_conns=1, conn_k=3)  # degree 4 does not fit q_deg = 2


@pytest.mark.parametrize("n_bits,k,blow", [(6, 1, 1), (8, 2, 1), (8, 3, 2), (7, 4, 2)])
def test_construction_closes_and_one_cell_breaks_two_links(oracle, n_bits, k, blow):
    import stark_verify as sv
    from oracle.stark_prover import OracleStark, to_json
    from zkgpu import synthetic as sy
    inst = sy.SyntheticStark(n_bits=n_bits, blowup_bits=blow, q_deg=max(2, k), n_conns=1, conn_k=k, n_queries=8)
    o = OracleStark(inst)
    o.witness()
    trace = o.S[0].copy()
    a, s, ks = _columns(inst, o, trace)
    # S is what conn_wiring says, cell by cell
    ids = cc.identities(ks, n_bits)
    n = 1 << n_bits
    for i, (j, rot) in enumerate(inst.conn_wiring(inst.conns[0])):
        assert [int(x) for x in s[i]] == [ids[j * n + (r + rot) % n] for r in range(n)]
    assert cc.reference(a, s, ks, n_bits, 16) == ((0, 0, 0), [], [])
    rng = np.random.default_rng(n_bits)
    beta, gamma = (int(x) for x in rng.integers(1, P, size=2, dtype=np.uint64))
    assert cc.closes(a, s, ks, n_bits, beta, gamma)
    bad = sv.verify(inst, to_json(o.prove()), o.verkey, o.publics)
    assert not sv.failures(bad), sv.failures(bad)
    clean = ac.audit(o, names=True)
    assert clean["clean"] == 1 and clean["identities"]["ran"] == 1
    if k == 1:
        return  # every cell is wired to itself: nothing can break
    row = n // 2 + 5
    o.S[0][row, inst.conns[0]["cols"][1]] = (int(trace[row, inst.conns[0]["cols"][1]]) + 1) % P
    a, s, ks = _columns(inst, o, o.S[0])
    counts, breaks, _ = cc.reference(a, s, ks, n_bits, 16)
    assert counts == (2, 0, 0) and all(n + row in b[:2] for b in breaks)
    assert not cc.closes(a, s, ks, n_bits, beta, gamma)
    rep = ac.audit(o, names=True)
    assert rep["clean"] == 0 and [e["z"] for e in rep["z"]] == [len(inst.z_ctx) - 1]
    assert rep["identities"]["ran"] == 1 and 1 <= rep["identities"]["n_bad"] <= 2


def test_starkinfo_lists_the_connection_under_ciCtx(tmp_path):
    import json

    import zkgpu.starkinfo as zs
    from zkgpu import synthetic as sy
    base = zs.starkinfo(sy.SyntheticStark(n_bits=6, t=2, m=1, n_queries=4))
    assert base["ciCtx"] == []
    inst = sy.SyntheticStark(n_bits=6, t=2, m=1, n_queries=4, n_conns=1)
    j = zs.starkinfo(inst)
    assert len(j["ciCtx"]) == 1 and len(j["puCtx"]) == 2 and len(j["peCtx"]) == 1
    cn = inst.conns[0]
    exp_col = lambda e: j["varPolMap"][j["exps_n"][e]]["sectionPos"]  # noqa: E731
    assert (exp_col(j["ciCtx"][0]["numId"]), exp_col(j["ciCtx"][0]["denId"])) == (cn["num"], cn["den"])
    # its Z is the committed polynomial after the cm1 columns, h1 / h2 and the Z of puCtx and peCtx
    zpol = j["varPolMap"][j["cm_n"][j["nCm1"] + 2 * 2 + 2 + 1]]
    assert (zpol["section"], zpol["sectionPos"], zpol["dim"]) == ("cm3_n", cn["z"], 3)
    assert any(op["src"][-1] == {"type": "x"} for op in j["step3prev"]["first"] if len(op["src"]) == 2)
    path = zs.write_connections(str(tmp_path / "c.json"), inst)
    assert json.load(open(path)) == [{"ciCtx": 0, "pols": cn["cols"], "S": cn["S"], "ks": ["1", "12"]}]
