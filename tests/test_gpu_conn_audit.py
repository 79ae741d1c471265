"""Connection checks in the prover (include/zkgpu_stark.h zkgpu_stark_conn_set /
conn_check / audit_conn) on the SyntheticStark instance with one connection
(n_conns = 1) at 2^10 rows: two columns at the default blowup, three columns
at blowup 4 once.  The GPU proof is the oracle's bit for bit and replays in the
verifier; a clean trace audits clean and queues no connection report; one cell
of a_1 off by one opens the connection's product and audit_conn / conn_check
name the two links that break, as the pure-Python reference
(tests/conn_cases.py); the audit's own report stays the oracle's
(tests/audit_cases.py) and, with no connection declared, its text is what it
was."""
import uuid

import numpy as np
import pytest

import audit_cases as ac
import conn_cases as cc

pytestmark = pytest.mark.gpu

N_BITS = 10
N = 1 << N_BITS
KEYS = ("clean", "challenges", "n_pu_bad", "pu", "n_z_open", "z", "identities")
ROW = 517  # the planted cell: a_1 at this row
SHAPES = {"k2": dict(n_conns=1), "k3": dict(n_conns=1, conn_k=3, blowup_bits=2, q_deg=3)}


@pytest.fixture(scope="module")
def world(oracle):
    """{shape: (instance, its OracleStark, the clean trace, the oracle's proof)}"""
    from oracle.stark_prover import OracleStark
    from zkgpu.synthetic import SyntheticStark
    out = {}
    for name, kw in SHAPES.items():
        inst = SyntheticStark(n_bits=N_BITS, **kw)
        o = OracleStark(inst)
        o.witness()
        out[name] = (inst, o, o.S[0].copy(), o.prove())
    return out


def planted(world, shape):
    inst, o, trace, _ = world[shape]
    bad = trace.copy()
    c = inst.conns[0]["cols"][1]
    bad[ROW, c] = (int(bad[ROW, c]) + 1) % cc.P
    return bad


_REF = {}


def audit_reference(world, shape, what, bad):
    """the oracle's audit of a trace, computed once per shape and trace"""
    if (shape, what) not in _REF:
        inst, o, trace, _ = world[shape]
        o.S[0][:] = bad
        _REF[(shape, what)] = ac.audit(o, names=True)
        o.S[0][:] = trace
    return _REF[(shape, what)]


def conn_reference(world, shape, trace, z):
    """the report of GpuStark.conn_check from the pure-Python reference"""
    inst, o, _, _ = world[shape]
    cn = inst.conns[0]
    a = np.ascontiguousarray(trace[:, cn["cols"]].T)
    s = np.ascontiguousarray(o.S[4][:, cn["S"]].T)
    counts, breaks, foreign = cc.reference(a, s, cn["ks"], N_BITS, 16)
    return {"ran": 1, "z": z, "n_broken": counts[0], "n_foreign": counts[1], "n_untargeted": counts[2],
            "breaks": [(c // N, c % N, t // N, t % N, v, tv) for c, t, v, tv in breaks],
            "foreign": [(c // N, c % N, v) for c, v in foreign]}


def declare(g, inst, z=None):
    cn = inst.conns[0]
    g.conn_set(len(inst.z_ctx) - 1 if z is None else z, cn["cols"], cn["S"])


def prover(inst):
    from zkgpu.stark import GpuStark
    return GpuStark(inst)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_proof_is_the_oracles_and_replays(zkgpu, world, shape):
    import stark_verify as sv
    from oracle.stark_prover import to_json
    inst, o, trace, proof = world[shape]
    assert len(inst.conns[0]["cols"]) == (3 if shape == "k3" else 2)
    bad = sv.verify(inst, to_json(proof), o.verkey, o.publics)
    assert not sv.failures(bad), sv.failures(bad)
    g = prover(inst)
    try:
        g.set_cm1(trace)
        assert g.prove() == proof
        g.witness()  # the GPU's own step1 builds the same trace
        assert np.array_equal(g.get_cm1(), trace)
    finally:
        g.close()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_clean_trace_audits_clean(zkgpu, world, shape):
    inst, o, trace, proof = world[shape]
    z = len(inst.z_ctx) - 1
    g = prover(inst)
    try:
        declare(g, inst)
        g.set_cm1(trace)
        got = g.audit(names=True)
        want = audit_reference(world, shape, "clean", trace)
        assert got["clean"] == 1 and {k: got[k] for k in KEYS} == {k: want[k] for k in KEYS}
        # layer C runs: the n-domain rewrite takes the connection's identities (x included)
        assert got["identities"]["ran"] == 1 and got["identities"]["n_bad"] == 0
        assert g.audit_conn(0)["ran"] == 0  # a closed product queues nothing
        assert "connection" not in g.audit_text()
        assert g.conn_check(z) == conn_reference(world, shape, trace, z)
        assert g.conn_check(z)["n_broken"] == 0
        assert g.prove() == proof
    finally:
        g.close()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_one_cell_off(zkgpu, world, shape):
    from zkgpu import ZkgpuError
    inst, o, trace, proof = world[shape]
    z, nz = len(inst.z_ctx) - 1, len(inst.z_ctx)
    bad = planted(world, shape)
    want_conn = conn_reference(world, shape, bad, z)
    assert want_conn["n_broken"] == 2 and want_conn["n_foreign"] == 0 and want_conn["n_untargeted"] == 0
    assert all((1, ROW) in (b[0:2], b[2:4]) for b in want_conn["breaks"])  # both name the planted cell
    want = audit_reference(world, shape, "planted", bad)
    g = prover(inst)
    try:
        g.set_cm1(bad)
        # no connection declared: today's audit and today's text
        got = g.audit(names=True)
        assert {k: got[k] for k in KEYS} == {k: want[k] for k in KEYS}
        assert [e["z"] for e in got["z"]] == [z] and got["clean"] == 0
        assert g.audit_conn(0)["ran"] == 0
        plain = g.audit_text()
        assert "connection" not in plain
        # the same declared: the report itself does not change, the connection's report goes with entry 0
        declare(g, inst)
        got = g.audit(names=True)
        assert {k: got[k] for k in KEYS} == {k: want[k] for k in KEYS}
        assert g.audit_conn(0) == want_conn
        assert g.audit_conn(1)["ran"] == 0
        text = g.audit_text()
        lines = text.splitlines()
        assert [l for l in lines if not l.startswith("  connection: ")] == plain.splitlines()
        b0, b1 = ((c, r, v, tc, tr, tv) for c, r, tc, tr, v, tv in want_conn["breaks"])
        at = [i for i, l in enumerate(lines) if l.startswith("calculateZ: grand product %d does not close" % z)][0]
        assert lines[at + 1] == ("  connection: 2 cell(s) differ from the cell they are wired to; pols[%d] row %d (= %d) "
                                 "is wired to pols[%d] row %d (= %d)" % b0)
        assert lines[at + 2] == "  connection: pols[%d] row %d (= %d) is wired to pols[%d] row %d (= %d)" % b1
        assert not lines[at + 3].startswith("  connection")
        # layer C: the product's boundary or transition identity fails on a row or two
        assert got["identities"]["ran"] == 1 and 1 <= got["identities"]["n_bad"] <= 2
        # the declaration cleared: the plain text again
        g.conn_set(z)
        g.audit(names=True)
        assert g.audit_text() == plain
        # the proof fails as it did
        with pytest.raises(ZkgpuError) as e:
            g.prove()
        assert str(e.value).startswith("zkgpu_stark_prove failed: calculateZ: grand product %d does not close (1 of %d "
                                       "do not): " % (z, nz))
        assert "connection" not in str(e.value) and "unmatched" in str(e.value)
    finally:
        g.close()
    # conn_check alone, on a prover that never audited
    g = prover(inst)
    try:
        declare(g, inst)
        g.set_cm1(bad)
        assert g.conn_check(z) == want_conn
        assert np.array_equal(g.get_cm1(), bad)  # the trace is untouched
        g.set_cm1(trace)
        assert g.prove() == proof
    finally:
        g.close()


def test_refusals(zkgpu, world):
    from zkgpu import ZkgpuError
    from zkgpu.stark import GpuStark, ShmComm
    inst, o, trace, proof = world["k2"]
    cn = inst.conns[0]
    z = len(inst.z_ctx) - 1
    comm = ShmComm("/zkgpu_conn_%s" % uuid.uuid4().hex[:12], 1, 0, capacity=1 << 20)
    try:
        g = GpuStark(inst, comm=comm)
        try:
            for call in (lambda: declare(g, inst), lambda: g.conn_check(z), lambda: g.audit_conn(0)):
                with pytest.raises(ZkgpuError, match="single-GPU provers only"):
                    call()
        finally:
            g.close()
    finally:
        comm.close()
    g = prover(inst)
    try:
        with pytest.raises(ZkgpuError, match="audit_conn: no audit has run"):
            g.audit_conn(0)
        with pytest.raises(ZkgpuError, match="conn_check: product %d is not declared a connection" % z):
            g.conn_check(z)
        with pytest.raises(ZkgpuError, match="conn_set: product %d: the instance has %d grand product" % (z + 1, z + 1)):
            g.conn_set(z + 1, cn["cols"], cn["S"])
        with pytest.raises(ZkgpuError, match="conn_set: product %d: cm1 column %d: the instance has %d"
                           % (z, inst.n_cm1, inst.n_cm1)):
            g.conn_set(z, [cn["cols"][0], inst.n_cm1], cn["S"])
        with pytest.raises(ZkgpuError, match="conn_set: product %d: constant column %d: the instance has %d"
                           % (z, inst.n_const, inst.n_const)):
            g.conn_set(z, cn["cols"], [inst.n_const, cn["S"][1]])
        with pytest.raises(ZkgpuError, match="conn_set: product %d: column %d repeated" % (z, cn["cols"][0])):
            g.conn_set(z, [cn["cols"][0]] * 2, cn["S"])
        with pytest.raises(ZkgpuError, match="the cosets of ks\\[0\\] and ks\\[1\\] collide"):
            g.conn_set(z, cn["cols"], cn["S"], ks=[3, 3 * cc.omega(N_BITS) % cc.P])
        with pytest.raises(ZkgpuError, match="conn_check: product %d: the instance has" % (z + 1)):
            g.conn_check(z + 1)
        declare(g, inst)
        with pytest.raises(ZkgpuError, match="conn_check: no trace is loaded"):
            g.conn_check(z)
        g.set_cm1(trace)
        assert g.conn_check(z)["n_broken"] == 0
        # other shifts than the constants were built with: every S value outside column 0's coset is foreign
        g.conn_set(z, cn["cols"], cn["S"], ks=[1, 7])
        r = g.conn_check(z)
        assert r["n_broken"] == 0 and r["n_foreign"] == N and r["n_untargeted"] == N
        assert r["foreign"] == [(0, row, int(o.S[4][row, cn["S"][0]])) for row in range(16)]
    finally:
        g.close()
