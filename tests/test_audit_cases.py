"""CPU side of the trace audit: the audit restated on the oracle
(tests/audit_cases.py) on a clean and on a broken SyntheticStark trace at 2^6
rows.  A clean trace gives a clean report; each planted fault is reported in
its own layer -- and only there, but for what the audit's contract says
follows from it: a plookup that missed leaves its own product open and stops
the identities, an open permutation product fails its boundary identities."""
import numpy as np
import pytest

import audit_cases as ac
import multiset_cases as mc

N_BITS = 6
N = 1 << N_BITS


@pytest.fixture(scope="module")
def world(oracle):
    from oracle.stark_prover import OracleStark
    from zkgpu.synthetic import SyntheticStark
    inst = SyntheticStark(n_bits=N_BITS, n_lookups=2, n_perms=1)
    o = OracleStark(inst)
    o.witness()
    return inst, o, o.S[0].copy()


def run(world, trace, names=False):
    inst, o, _ = world
    o.S[0][:] = trace
    return ac.audit(o, names=names)


def test_challenges_come_from_verkey_and_publics_alone(world, oracle):
    inst, o, clean = world
    t = oracle.Transcript()
    t.put(o.verkey)
    t.put(o.publics)
    want = [int(x) for _ in range(5) for x in t.get_field()]
    bad = ac.plant(inst, clean, identity_rows=[3])
    assert run(world, clean)["challenges"] == want == run(world, bad)["challenges"]
    assert len(want) == 15 and want[12:] == run(world, clean)["identities"]["alpha"]


def test_clean_trace_gives_a_clean_report(world):
    inst, o, clean = world
    r = run(world, clean, names=True)
    assert r["clean"] == 1 and r["n_pu_bad"] == 0 and r["pu"] == [] and r["n_z_open"] == 0 and r["z"] == []
    assert r["identities"]["ran"] == 1 and r["identities"]["n_bad"] == 0 and r["identities"]["rows"] == []
    assert r["named"] == []
    # the audit left what a proof needs: the same trace proves as before
    o.S[0][:] = clean
    first = o.prove()
    run(world, clean)
    assert o.prove() == first


def test_identity_fault_is_reported_by_layer_c_alone(world):
    inst, o, clean = world
    rows = [0, 37, N - 1]
    r = run(world, ac.plant(inst, clean, identity_rows=rows), names=True)
    assert r["clean"] == 0 and r["n_pu_bad"] == 0 and r["n_z_open"] == 0
    assert r["identities"]["ran"] == 1 and r["identities"]["rows"] == rows and r["identities"]["n_bad"] == 3
    assert any(r["identities"]["value"])
    ids = [ids for ids, _ in r["named"]]
    assert len(ids) == 3 and ids[0] and ids[0] == ids[1] == ids[2]  # the same identity at each row


def test_permutation_fault_is_reported_by_layer_b(world):
    inst, o, clean = world
    bad = ac.plant(inst, clean, perm_cells=[(21, 2)])
    r = run(world, bad, names=True)
    z = len(inst.z_ctx) - 1
    assert r["clean"] == 0 and r["n_pu_bad"] == 0 and r["n_z_open"] == 1
    want = mc.perm_reference(inst, bad)
    assert r["z"] == [dict(z=z, compared=1, **want)]
    assert want == {"n_num": 1, "num": [((21 + inst.PERM_ROT) % N, 1, 0)], "n_den": 1, "den": [(21, 0, 1)]}
    # the open product does not stop layer C: its boundary identity fails, on a row or two, and nothing else does
    assert r["identities"]["ran"] == 1 and 1 <= r["identities"]["n_bad"] <= 2
    clean_ids = set()
    for ids, _ in run(world, ac.plant(inst, clean, identity_rows=[5]), names=True)["named"]:
        clean_ids |= set(ids)
    for ids, _ in r["named"]:
        assert ids and not set(ids) & clean_ids


@pytest.mark.parametrize("pu", [0, 1])
def test_lookup_fault_is_reported_by_layer_a(world, pu):
    inst, o, clean = world
    v = ac.absent_value(inst, o)
    m = len(inst.z_ctx) - len(inst.lookups) - len(inst.perms)  # the products ahead of the plookups'
    for cells, want in (([(pu, 17, v)], (1, 1, [(17, 1)])),
                        ([(pu, 17, v), (pu, 40, v)], (2, 1, [(17, 2)])),
                        ([(pu, 0, v), (pu, N - 1, v + 1)], (2, 2, [(0, 1), (N - 1, 1)]))):
        r = run(world, ac.plant(inst, clean, lookup_cells=cells), names=True)
        assert r["clean"] == 0 and r["n_pu_bad"] == 1
        assert r["pu"] == [{"pu": pu, "n_rows": want[0], "n_vals": want[1], "vals": want[2]}]
        # its own product is open (h1 / h2 read zero), no other; the identities did not run
        assert r["n_z_open"] == 1 and r["z"][0]["z"] == m + pu
        assert r["identities"]["ran"] == 0 and r["identities"]["n_bad"] == 0 and "named" not in r


def test_all_faults_at_once(world):
    inst, o, clean = world
    v = ac.absent_value(inst, o)
    bad = ac.plant(inst, clean, identity_rows=[0, 37], perm_cells=[(21, 2)],
                   lookup_cells=[(0, 17, v), (1, 17, v), (1, 40, v)])
    r = run(world, bad)
    m = len(inst.z_ctx) - len(inst.lookups) - len(inst.perms)
    assert r["clean"] == 0 and r["n_pu_bad"] == 2 and [e["pu"] for e in r["pu"]] == [0, 1]
    assert [(e["n_rows"], e["n_vals"], e["vals"]) for e in r["pu"]] == [(1, 1, [(17, 1)]), (2, 1, [(17, 2)])]
    assert r["n_z_open"] == 3 and [e["z"] for e in r["z"]] == [m, m + 1, len(inst.z_ctx) - 1]
    assert r["z"][2]["den"] == [(21, 0, 1)]
    assert r["identities"]["ran"] == 0
