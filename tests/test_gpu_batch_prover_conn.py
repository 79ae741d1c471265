"""zkgpu_batch_prover --audit --connections on written instance files: the
starkinfo's ciCtx entry and the sidecar of a SyntheticStark with one
connection, one cell of a_1 off by one.  The report names the two links that
break with pols[i] beside the cm1 column, on stdout under the product's line
and on stderr, trace_audit.json carries them, the exit status is the audit's;
without the sidecar the report is what it was; a malformed sidecar is refused
by the entry's index, and the option is refused without --audit."""
import json
import subprocess

import numpy as np
import pytest

import conn_cases as cc
from test_starkinfo import DRIVER

pytestmark = pytest.mark.gpu

N_BITS = 8
N = 1 << N_BITS
ROW = 77


@pytest.fixture(scope="module")
def world(oracle):
    from oracle.stark_prover import OracleStark
    from zkgpu.synthetic import SyntheticStark
    inst = SyntheticStark(n_bits=N_BITS, t=2, m=1, n_queries=8, n_conns=1)
    o = OracleStark(inst)
    o.witness()
    bad = o.S[0].copy()
    c = inst.conns[0]["cols"][1]
    bad[ROW, c] = (int(bad[ROW, c]) + 1) % cc.P
    return inst, o, o.S[0].copy(), bad


def _run(world, tmp_path, trace, *opts):
    import zkgpu.starkinfo as zs
    inst, o, _, _ = world
    cfg = zs.write_inputs(str(tmp_path), inst, o.S[4], o.S[9], o.const_nodes, trace, o.publics)
    r = subprocess.run([DRIVER, *opts, cfg], capture_output=True, text=True, timeout=300)
    return r, tmp_path / "out"


def _sidecar(world, tmp_path, entries=None):
    import zkgpu.starkinfo as zs
    path = str(tmp_path / "connections.json")
    if entries is None:
        return zs.write_connections(path, world[0])
    with open(path, "w") as f:
        json.dump(entries, f)
    return path


def test_starkinfo_and_sidecar(world, tmp_path):
    import zkgpu.starkinfo as zs
    inst = world[0]
    j = zs.starkinfo(inst)
    assert len(j["ciCtx"]) == 1 and set(j["ciCtx"][0]) == {"zId", "numId", "denId", "c1Id", "c2Id"}
    cn = inst.conns[0]
    assert zs.connections(inst) == [{"ciCtx": 0, "pols": cn["cols"], "S": cn["S"], "ks": ["1", "12"]}]
    # the driver's loader puts the connection's triple last: puCtx, peCtx, ciCtx
    zs.write_inputs(str(tmp_path), inst, world[1].S[4], world[1].S[9], world[1].const_nodes, world[2], world[1].publics)
    d = json.loads(subprocess.run([DRIVER, "--info", str(tmp_path / "zkevm.starkinfo.json")], capture_output=True,
                                  text=True, timeout=120).stdout)
    assert tuple(d["zCtx"][-3:]) == (cn["num"], cn["den"], cn["z"]) == tuple(inst.z_ctx[-1])


def test_planted_cell_is_named(world, tmp_path):
    inst, o, clean, bad = world
    cn = inst.conns[0]
    z = len(inst.z_ctx) - 1  # (ciCtx comes last in the driver's order too)
    counts, breaks, _ = cc.reference(np.ascontiguousarray(bad[:, cn["cols"]].T),
                                     np.ascontiguousarray(o.S[4][:, cn["S"]].T), cn["ks"], N_BITS, 16)
    assert counts == (2, 0, 0)
    plain, _ = _run(world, tmp_path, bad, "--audit")
    assert plain.returncode == 3 and "connection:" not in plain.stdout + plain.stderr, (plain.stdout, plain.stderr)
    r, out = _run(world, tmp_path, bad, "--audit", "--connections", _sidecar(world, tmp_path))
    assert r.returncode == 3, (r.returncode, r.stdout, r.stderr)

    def link(c, t, v, tv):
        return "pols[%d] (cm1 column %d) row %d (= %d) is wired to pols[%d] (cm1 column %d) row %d (= %d)" % (
            c // N, cn["cols"][c // N], c % N, v, t // N, cn["cols"][t // N], t % N, tv)

    want = ["  connection: 2 cell(s) differ from the cell they are wired to; " + link(*breaks[0]),
            "  connection: " + link(*breaks[1])]
    assert any("row %d " % ROW in l for l in want)
    lines = r.stdout.splitlines()
    at = [i for i, l in enumerate(lines) if l.startswith("calculateZ: grand product %d does not close" % z)][0]
    assert "grand product %d is connection check 0 (ciCtx[0])" % z in lines[at]
    assert lines[at + 1:at + 3] == want
    assert [l for l in lines if not l.startswith("  connection: ")] == plain.stdout.splitlines()
    err = r.stderr.splitlines()
    at = err.index("zkgpu_batch_prover: grand product %d is connection check 0 (ciCtx[0])" % z)
    assert err[at + 1:at + 3] == want
    got = json.loads((out / "trace_audit.json").read_text())
    e = [e for e in got["z"] if e["z"] == z][0]
    assert e["context"] == "connection check 0 (ciCtx[0])"
    assert (e["connection"]["n_broken"], e["connection"]["n_foreign"], e["connection"]["n_untargeted"]) == counts
    assert [(b[0] * N + b[1], b[2] * N + b[3], int(b[4]), int(b[5])) for b in e["connection"]["breaks"]] == breaks
    assert e["connection"]["foreign"] == []


def test_clean_trace(world, tmp_path):
    inst, o, clean, bad = world
    r, out = _run(world, tmp_path, clean, "--audit", "--connections", _sidecar(world, tmp_path))
    assert r.returncode == 0 and "connection:" not in r.stdout + r.stderr, (r.stdout, r.stderr)
    assert "connection" not in (out / "trace_audit.json").read_text()


def test_malformed_sidecars_are_refused_by_entry(world, tmp_path):
    inst, o, clean, bad = world
    cn = inst.conns[0]
    good = {"ciCtx": 0, "pols": cn["cols"], "S": cn["S"]}
    for entries, message in (
            ([good, dict(good, ciCtx=1)], "--connections: entry 1: ciCtx 1: the starkinfo has 1 connection check(s)"),
            ([good, good], "--connections: entry 1: ciCtx 0 is declared twice"),
            ([dict(good, pols=cn["cols"][:1])],
             '--connections: entry 0: "pols", "S" and "ks" must be lists of one length, not empty (1, 2)'),
            ([dict(good, ks=["1"])],
             '--connections: entry 0: "pols", "S" and "ks" must be lists of one length, not empty (2, 2, 1)'),
            ([{"ciCtx": 0, "S": cn["S"]}], '--connections: entry 0: json: missing key "pols"'),
            ([dict(good, pols=[cn["cols"][0], inst.n_cm1])],
             "--connections: entry 0: conn_set: product %d: cm1 column %d: the instance has %d"
             % (len(inst.z_ctx) - 1, inst.n_cm1, inst.n_cm1)),
            ([dict(good, ks=["5", "0"])], "--connections: entry 0: conn_set: product %d: conn_breaks: ks[1] is zero"
             % (len(inst.z_ctx) - 1)),
            ({"ciCtx": 0}, "--connections: %s: not a list of entries" % str(tmp_path / "connections.json"))):
        r, out = _run(world, tmp_path, clean, "--audit", "--connections", _sidecar(world, tmp_path, entries))
        assert r.returncode == 1 and r.stderr.strip().endswith(message), (r.returncode, r.stderr, message)
        assert not (out / "trace_audit.json").exists()
    r, out = _run(world, tmp_path, clean, "--connections", _sidecar(world, tmp_path))
    assert r.returncode == 1 and "--connections names the wiring for --audit: not without it" in r.stderr
