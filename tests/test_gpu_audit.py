"""The trace audit (include/zkgpu_stark.h zkgpu_stark_audit) against its
restatement on the oracle (tests/audit_cases.py), word for word: the
SyntheticStark instance with two plookups and one permutation check at 2^10
rows, blowup 1 and 2, under both memory plans.  A clean trace is clean and
proves as the oracle right after; one fault per layer, and all at once, give
the reference's report; the audit launches nothing of an LDE, a tree, a FRI
fold or an opening."""
import uuid

import numpy as np
import pytest

import audit_cases as ac

pytestmark = pytest.mark.gpu

N_BITS = 10
N = 1 << N_BITS
KEYS = ("clean", "challenges", "n_pu_bad", "pu", "n_z_open", "z", "identities")


@pytest.fixture(scope="module")
def world(oracle):
    """{blowup bits: (instance, its OracleStark, the clean trace, the oracle's proof, an absent lookup value)}"""
    from oracle.stark_prover import OracleStark
    from zkgpu.synthetic import SyntheticStark
    out = {}
    for blow in (1, 2):
        inst = SyntheticStark(n_bits=N_BITS, blowup_bits=blow, n_lookups=2, n_perms=1)
        o = OracleStark(inst)
        o.witness()
        trace = o.S[0].copy()
        out[blow] = (inst, o, trace, o.prove(), ac.absent_value(inst, o))
    return out


def faults(v):
    """name -> plant() arguments: one fault per layer, then all of them"""
    f = {"identity": dict(identity_rows=[0, 517, N - 1]),
         "permutation": dict(perm_cells=[(517, 2)])}
    for pu in (0, 1):
        f["plookup%d_one_row" % pu] = dict(lookup_cells=[(pu, 17, v)])
        f["plookup%d_two_rows" % pu] = dict(lookup_cells=[(pu, 17, v), (pu, 900, v)])
    f["all"] = dict(identity_rows=[0, 517, N - 1], perm_cells=[(517, 2)],
                    lookup_cells=[(0, 17, v), (1, 17, v), (1, 900, v)])
    return f


_REF = {}


def reference(world, blow, name):
    """(the altered trace, the reference's report), computed once per blowup and fault"""
    if (blow, name) not in _REF:
        inst, o, trace, _, v = world[blow]
        bad = trace if name == "clean" else ac.plant(inst, trace, **faults(v)[name])
        o.S[0][:] = bad
        _REF[(blow, name)] = (bad, ac.audit(o, names=True))
        o.S[0][:] = trace
    return _REF[(blow, name)]


def _modes():
    from zkgpu.stark import MEM_LEAN, MEM_RESIDENT
    return {"resident": MEM_RESIDENT, "lean": MEM_LEAN}


def _prover(world, blow, mode, monkeypatch):
    from zkgpu.stark import GpuStark
    monkeypatch.delenv("ZKGPU_LEAN_KEEP_COLS", raising=False)
    return GpuStark(world[blow][0], mode=_modes()[mode])


def _same(g, got, want, named=True):
    assert {k: got[k] for k in KEYS} == {k: want[k] for k in KEYS}
    # the earlier diagnoses' readers refer to the audit
    assert g.check_result() == got["identities"]
    d = g.z_diag()
    if got["n_z_open"]:
        z0 = got["z"][0]
        assert (d["ran"], d["z"], d["n_open"]) == (1, z0["z"], got["n_z_open"])
        assert {k: d[k] for k in ("n_num", "n_den", "num", "den")} == {k: z0[k] for k in ("n_num", "n_den", "num", "den")}
    else:
        assert d["ran"] == 0 and d["n_open"] == 0
    if named and got["identities"]["ran"]:
        for slot, (ids, vals) in enumerate(want["named"]):
            assert g.check_named(slot) == (ids, vals, len(ids)), slot
        if len(want["named"]) < 16:  # a slot past the last failing row is empty
            assert g.check_named(len(want["named"]))[2] == 0


def _audit_timers(g, pu=True):
    t = g.timers()
    assert not [k for k in t if k.startswith("STARK_STEP_")], t
    assert {"AUDIT_STEP2", "AUDIT_STEP3PREV", "AUDIT_Z", "AUDIT_TOTAL"} <= set(t), t
    assert ("AUDIT_H1H2" in t) == pu
    assert all(k.startswith("AUDIT_") for k in t), t
    return t


@pytest.mark.parametrize("mode", ["resident", "lean"])
@pytest.mark.parametrize("blow", [1, 2])
def test_clean_trace_then_the_proof(zkgpu, world, monkeypatch, blow, mode):
    inst, o, trace, proof, _ = world[blow]
    _, want = reference(world, blow, "clean")
    g = _prover(world, blow, mode, monkeypatch)
    try:
        g.set_cm1(trace)
        got = g.audit(names=True)
        assert got["clean"] == 1 and got["challenges"] == want["challenges"]
        _same(g, got, want)
        t = _audit_timers(g)
        assert {"AUDIT_STEP3", "AUDIT_CONSTRAINTS"} <= set(t)
        text = g.audit_text()
        assert "clean" in text.splitlines()[0] and "NOT clean" not in text
        assert "every identity holds" in text
        # no reload: the audit consumed nothing, under the lean plan too
        assert g.prove() == proof
        assert any(k.startswith("STARK_STEP_") for k in g.timers())
        if mode == "resident":  # the trace outlives the proof: audit and prove again
            assert g.audit()["clean"] == 1
            assert g.prove() == proof
    finally:
        g.close()


def test_audit_launches_no_commitment_kernel(zkgpu, world, monkeypatch):
    """a condition, no number: what a clean audit launches is part of what a checked proof launches,
    and none of it is a kernel of the LDE, the tree, the FRI fold or the openings"""
    from zkgpu.stark import CHECK_REPORT
    inst, o, trace, proof, _ = world[1]
    ne = 2 * N
    g = _prover(world, 1, "resident", monkeypatch)
    zkgpu.prof_enable(True)
    try:
        g.set_cm1(trace)
        assert g.audit(names=True)["clean"] == 1  # (the first use compiles the rewritten step42ns)
        zkgpu.prof_reset()
        assert g.audit(names=True)["clean"] == 1
        audit = set(zkgpu.prof_kernels())
        g.check_set(CHECK_REPORT)
        g.check_names_set(True)
        zkgpu.prof_reset()
        assert g.prove() == proof
        checked = set(zkgpu.prof_kernels())
        print("audit", sorted(audit))
        print("checked proof", sorted(checked))
        assert audit and audit <= checked, sorted(audit - checked)
        # each commitment primitive alone at that shape
        rng = np.random.default_rng(7)
        ncols = inst.n_cm1
        src = zkgpu.to_device(rng.integers(0, ac.P, size=ncols * N, dtype=np.uint64))
        ext = zkgpu.to_device(np.zeros(ncols * ne, np.uint64))
        nodes = zkgpu.to_device(np.zeros(int(zkgpu.lib().zkgpu_gl_merkle_num_elements(ne)), np.uint64))
        pol = zkgpu.to_device(rng.integers(0, ac.P, size=3 * ne, dtype=np.uint64))
        folded = zkgpu.to_device(np.zeros(3 * (ne >> 4), np.uint64))
        alone = {}

        def profiled(name, f):
            zkgpu.synchronize()
            zkgpu.prof_reset()
            f()
            zkgpu.synchronize()
            alone[name] = set(zkgpu.prof_kernels())
            print(name, sorted(alone[name]))

        profiled("zkgpu_gl_extend_pol_dev", lambda: zkgpu.extend_pol_dev(ext, ne, src, N, ne, N, ncols))
        profiled("zkgpu_gl_merkletree_dev", lambda: zkgpu.merkletree_dev(nodes, ext, ne, ncols, ne))
        profiled("zkgpu_fri_fold_dev", lambda: zkgpu.fri_fold_dev(
            folded, pol, N_BITS + 1, N_BITS + 1 - 4, rng.integers(0, ac.P, size=3, dtype=np.uint64), 7))
        profiled("zkgpu_gl_merkle_open_many", lambda: zkgpu.merkle_open_many(
            [(nodes, ext, ne, ncols, ne, np.arange(16, dtype=np.uint64) * 31, False)]))
        # (the openings' gathers take no profile record: their set may be empty, the others' are not)
        assert all(alone[k] for k in ("zkgpu_gl_extend_pol_dev", "zkgpu_gl_merkletree_dev", "zkgpu_fri_fold_dev"))
        for name, ks in alone.items():
            assert not audit & ks, (name, sorted(audit & ks))
    finally:
        zkgpu.prof_enable(False)
        g.close()


@pytest.mark.parametrize("mode", ["resident", "lean"])
@pytest.mark.parametrize("blow", [1, 2])
def test_one_fault_per_layer_and_all_at_once(zkgpu, world, monkeypatch, blow, mode):
    from zkgpu import ZkgpuError
    inst, o, trace, proof, v = world[blow]
    m = len(inst.z_ctx) - len(inst.lookups) - len(inst.perms)  # the products ahead of the plookups'
    g = _prover(world, blow, mode, monkeypatch)
    try:
        for name in faults(v):
            bad, want = reference(world, blow, name)
            g.set_cm1(bad)
            got = g.audit(names=True)
            print(name, got["n_pu_bad"], got["n_z_open"], got["identities"]["ran"], got["identities"]["n_bad"])
            assert got["clean"] == 0, name
            _same(g, got, want)
            text = g.audit_text()
            assert "NOT clean" in text.splitlines()[0], text
            if name == "identity":
                assert (got["n_pu_bad"], got["n_z_open"]) == (0, 0)
                assert got["identities"]["rows"] == [0, 517, N - 1] and got["identities"]["n_bad"] == 3
                assert "3 of the 2^10 = 1024 rows of the trace break the AIR; the first is row 0" in text
                assert "row 517: failing terms:" in text
            elif name == "permutation":
                assert got["n_pu_bad"] == 0 and [e["z"] for e in got["z"]] == [len(inst.z_ctx) - 1]
                assert got["z"][0]["den"] == [(517, 0, 1)] and got["z"][0]["num"] == [(517 + inst.PERM_ROT, 1, 0)]
                assert got["identities"]["ran"] == 1 and 1 <= got["identities"]["n_bad"] <= 2
                assert "calculateZ: grand product %d does not close (1 of %d do not): 1 value(s) of num unmatched, " \
                       "the first at row %d (1 in num, 0 in den); 1 value(s) of den unmatched, the first at row 517 " \
                       "(0 in num, 1 in den)" % (len(inst.z_ctx) - 1, len(inst.z_ctx), 517 + inst.PERM_ROT) in text
            elif name.startswith("plookup"):
                pu = int(name[7])
                rows = 1 if name.endswith("one_row") else 2
                assert got["pu"] == [{"pu": pu, "n_rows": rows, "n_vals": 1, "vals": [(17, rows)]}]
                assert [e["z"] for e in got["z"]] == [m + pu] and got["identities"]["ran"] == 0
                assert "Polinomial::calculateH1H2() Number not included: w=17 plookup_number=%d" % pu in text
            else:
                assert got["n_pu_bad"] == 2 and got["n_z_open"] == 3 and got["identities"]["ran"] == 0
                assert [(e["pu"], e["n_rows"], e["n_vals"], e["vals"]) for e in got["pu"]] == \
                    [(0, 1, 1, [(17, 1)]), (1, 2, 1, [(17, 2)])]
                assert "constraint check: not run: a plookup missed" in text
                assert "plookup_number=0" in text and "plookup_number=1" in text
                assert "grand product %d does not close (3 of %d do not)" % (len(inst.z_ctx) - 1, len(inst.z_ctx)) in text
        # the dirty trace still fails its proof as it did, at the first finding
        with pytest.raises(ZkgpuError) as e:
            g.prove()
        assert str(e.value) == ("zkgpu_stark_prove failed: Polinomial::calculateH1H2() Number not included: w=17 "
                                "plookup_number=0")
        # and the prover proves: the clean trace, the oracle's proof
        g.set_cm1(trace)
        assert g.prove() == proof
    finally:
        g.close()


def test_rows_only_without_names(zkgpu, world, monkeypatch):
    from zkgpu import ZkgpuError
    bad, want = reference(world, 1, "identity")
    g = _prover(world, 1, "resident", monkeypatch)
    try:
        g.set_cm1(bad)
        got = g.audit()
        _same(g, got, want, named=False)
        with pytest.raises(ZkgpuError, match="ran no check with naming on"):
            g.check_named(0)
        assert "failing terms" not in g.audit_text() and "  row 517\n" in g.audit_text()
        # the report is the audit's: a later proof (this trace's completes) does not change its text
        g.audit(names=True)
        text = g.audit_text()
        g.prove_raw()
        assert "  row 517: failing terms:" in text and g.audit_text() == text
    finally:
        g.close()


def test_refusals(zkgpu, world, monkeypatch):
    from zkgpu import ZkgpuError
    from zkgpu.stark import GpuStark, ShmComm
    inst, o, trace, proof, _ = world[1]
    comm = ShmComm("/zkgpu_aud_%s" % uuid.uuid4().hex[:12], 1, 0, capacity=1 << 20)
    try:
        g = GpuStark(inst, comm=comm)
        try:
            with pytest.raises(ZkgpuError, match="single-GPU provers only"):
                g.audit()
            with pytest.raises(ZkgpuError, match="single-GPU provers only"):
                g.audit_text()
        finally:
            g.close()
    finally:
        comm.close()
    for mode in ("resident", "lean"):
        g = _prover(world, 1, mode, monkeypatch)
        try:
            with pytest.raises(ZkgpuError, match="audit_format: no audit has run"):
                g.audit_text()
            with pytest.raises(ZkgpuError, match="audit: no trace is loaded"):
                g.audit()
            g.set_cm1(trace)
            assert g.prove() == proof
            if mode == "lean":
                with pytest.raises(ZkgpuError, match="audit: the previous proof consumed the trace"):
                    g.audit()
                g.set_cm1(trace)
            assert g.audit()["clean"] == 1
        finally:
            g.close()
