"""CPU side of the calculateZ diagnosis: the multiset reference on its case
table (tests/multiset_cases.py), the SyntheticStark permutation checks
(n_perms) through the oracle prover and the verifier replay, and the
workspace formula of zkgpu_multiset_diff_dev (host only)."""
import numpy as np
import pytest

import multiset_cases as mc
import stark_verify as sv


@pytest.mark.parametrize("dim", [1, 3])
@pytest.mark.parametrize("n", mc.SIZES)
def test_reference_on_case_table(n, dim):
    names = set()
    for case in mc.cases(n, dim):
        names.add(case.name)
        ref = case.reference()
        assert case.expect is not None, case.name
        n_a, la, n_b, lb = case.expect
        assert ref == (n_a, la[:case.max_vals], n_b, lb[:case.max_vals]), case.name
        words = mc.out_words(ref, case.max_vals)
        assert words.size == 2 * (1 + 3 * case.max_vals)
        # a permutation of a: two zero counts, padded lists
        if case.name.startswith("permuted") or case.name in ("same_pointer", "canonical"):
            assert ref == (0, [], 0, []) and set(words[1:1 + 3 * case.max_vals:3].tolist()) == {2**64 - 1}
    assert {"permuted_distinct", "same_pointer", "one_changed_row0", "one_changed_middle", "one_changed_last",
            "canonical", "all_distinct_16", "all_distinct_4096", "counts_only"} <= names
    if n >= 8:
        assert {"permuted_repeats", "three_against_two"} <= names
    if dim == 3 and n >= 2:
        assert "last_component" in names
    if n == 1 << 16:
        assert "selector" in names


def test_reference_small_by_hand():
    a = np.array([5, 7, 5, 9], np.uint64)
    b = np.array([7, 5, 11, 11], np.uint64)
    # 5: 2 against 1 (both sides); 9: a only; 11: b only, twice
    assert mc.reference(a, b, 16) == (2, [(0, 2, 1), (3, 1, 0)], 2, [(1, 2, 1), (2, 0, 2)])
    assert mc.reference(a, b, 1) == (2, [(0, 2, 1)], 2, [(1, 2, 1)])
    assert mc.reference(a, a + np.uint64(mc.P), 4) == (0, [], 0, [])


@pytest.fixture(scope="module")
def perm_proved(oracle):
    from oracle.stark_prover import OracleStark
    from zkgpu import synthetic as sy
    inst = sy.SyntheticStark(n_bits=10, n_perms=1)
    o = OracleStark(inst)
    o.witness()
    return inst, o, o.prove()


def test_permutation_instance_proves_and_verifies(perm_proved, oracle):
    inst, o, proof = perm_proved
    assert len(inst.perms) == 1 and inst.z_ctx[-1] == (inst.perms[0]["num"], inst.perms[0]["den"], inst.perms[0]["z"])
    bad = sv.verify(inst, proof, o.verkey, o.publics)
    assert not sv.failures(bad), bad
    _, _, ch = sv.gr.verify_fri(oracle, proof, [int(v) for v in o.verkey], [int(v) for v in o.publics],
                                list(inst.fri_steps), inst.n_queries)
    cz, q = sv.quotient_identity(inst, proof, ch, o.publics)
    assert cz == q and any(q)
    # the identity reads the permutation's Z: a changed eval of it breaks it
    i = inst.ev_index[(3 + 4, inst.perms[0]["z"], 1)]
    assert inst.evmap[i][0] == 7  # SEC_CM3_2NS
    p = dict(proof)
    p["evals"] = [list(e) for e in proof["evals"]]
    p["evals"][i][0] = str((int(p["evals"][i][0]) + 1) % sv.P)
    cz, q = sv.quotient_identity(inst, p, ch, o.publics)
    assert cz != q


def test_permutation_trace_is_a_rotation(perm_proved):
    inst, o, _ = perm_proved
    a, b, c, d = inst.perms[0]["cols"]
    cm1 = o.S[0]
    assert np.array_equal(cm1[:, c], np.roll(cm1[:, a], -inst.PERM_ROT))
    assert np.array_equal(cm1[:, d], np.roll(cm1[:, b], -inst.PERM_ROT))
    assert len(set(cm1[:, a].tolist())) == cm1.shape[0]  # distinct values: one altered cell is one orphan
    ref = mc.perm_reference(inst, cm1)
    assert ref == {"n_num": 0, "num": [], "n_den": 0, "den": []}
    bad = cm1.copy()
    bad[517, c] ^= np.uint64(1)
    r = int(np.where(cm1[:, a] == cm1[517, c])[0][0])
    assert mc.perm_reference(inst, bad) == {"n_num": 1, "num": [(r, 1, 0)], "n_den": 1, "den": [(517, 0, 1)]}


def test_default_instance_is_unchanged_by_n_perms():
    from zkgpu import synthetic as sy
    for kw in ({}, {"n_bits": 8, "n_lookups": 1, "n_free": 3, "n_free2": 2, "n_free3": 2, "n_free_tmp": 2}):
        x, y = sy.SyntheticStark(**kw), sy.SyntheticStark(n_perms=0, **kw)
        assert x.info() == y.info() and x.perms == []
        for name in x.programs:
            for u, v in zip(x.programs[name].arrays(), y.programs[name].arrays()):
                assert np.array_equal(u, v), name
            assert (x.programs[name].n_tmp1, x.programs[name].n_tmp3) == \
                (y.programs[name].n_tmp1, y.programs[name].n_tmp3)


def test_workspace_bytes_formula():
    import zkgpu
    f = zkgpu.multiset_diff_workspace_bytes
    assert f(0) <= 1 << 17
    prev = f(0)
    for n in [1, 2, 3, 255, 256, 257, 1000, 1024, 1025, 4097, 1 << 16, (1 << 16) + 1, 1 << 23, 1 << 28]:
        m = 1
        while m < 4 * n:
            m <<= 1
        blocks = (n + 1023) // 1024
        assert f(n) == 16 * m + 16 * n + 8 * ((blocks + 1) // 2) + 16 * 4097, n
        assert f(n) >= prev, n
        prev = f(n)


def test_starkinfo_writes_the_permutation_as_peCtx_0(tmp_path):
    """the driver's loader recovers the triples in the order puCtx, peCtx, ciCtx: the instance's
    permutation check is peCtx[0], ahead of the products of the h columns"""
    import json
    import zkgpu.starkinfo as zs
    from zkgpu import synthetic as sy
    from test_starkinfo import driver
    inst = sy.SyntheticStark(n_bits=6, t=2, m=1, n_queries=4, n_perms=1)
    j = zs.starkinfo(inst)
    assert len(j["puCtx"]) == 2 and len(j["peCtx"]) == 2
    path = tmp_path / "s.starkinfo.json"
    path.write_text(json.dumps(j))
    d = json.loads(driver("--info", str(path)).stdout)
    z = [tuple(d["zCtx"][i:i + 3]) for i in range(0, len(d["zCtx"]), 3)]
    pe = inst.perms[0]
    assert z[2] == (pe["num"], pe["den"], pe["z"]) and z[3] == inst.z_ctx[0]
    assert sorted(z) == sorted(inst.z_ctx)
