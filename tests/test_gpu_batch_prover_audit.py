"""zkgpu_batch_prover --audit on written instance files: the report with each
finding's starkinfo context on stdout, trace_audit.json against the audit's
restatement on the oracle (tests/audit_cases.py), the exit status, no proof
file, and the refusal with --shard at WORLD > 1."""
import json
import os
import subprocess

import pytest

import audit_cases as ac
from test_starkinfo import DRIVER

pytestmark = pytest.mark.gpu

N_BITS = 8
N = 1 << N_BITS


@pytest.fixture(scope="module")
def world(oracle):
    from oracle.stark_prover import OracleStark
    from zkgpu.synthetic import SyntheticStark
    inst = SyntheticStark(n_bits=N_BITS, t=2, m=1, n_queries=8, n_perms=1)
    o = OracleStark(inst)
    o.witness()
    return inst, o, o.S[0].copy()


def _run(world, tmp_path, trace, *opts):
    import zkgpu.starkinfo as zs
    inst, o, _ = world
    cfg = zs.write_inputs(str(tmp_path), inst, o.S[4], o.S[9], o.const_nodes, trace, o.publics)
    r = subprocess.run([DRIVER, *opts, cfg], capture_output=True, text=True, timeout=300)
    return r, tmp_path / "out"


def _reference(world, tmp_path, trace):
    """the oracle's report with the products renumbered as the driver orders them (puCtx, peCtx, ciCtx)"""
    inst, o, clean = world
    o.S[0][:] = trace
    want = ac.audit(o, names=True)
    o.S[0][:] = clean
    d = json.loads(subprocess.run([DRIVER, "--info", str(tmp_path / "zkevm.starkinfo.json")], capture_output=True,
                                  text=True, timeout=120).stdout)
    order = [tuple(d["zCtx"][i:i + 3]) for i in range(0, len(d["zCtx"]), 3)]
    for e in want["z"]:
        e["z"] = order.index(tuple(inst.z_ctx[e["z"]]))
    want["z"].sort(key=lambda e: e["z"])
    return want


def _same(got, want):
    assert got["clean"] == want["clean"]
    assert [int(x) for x in got["challenges"]] == want["challenges"]
    assert got["n_pu_bad"] == want["n_pu_bad"] and got["n_z_open"] == want["n_z_open"]
    assert [(e["pu"], e["n_rows"], e["n_vals"], [tuple(v) for v in e["vals"]]) for e in got["pu"]] == \
        [(e["pu"], e["n_rows"], e["n_vals"], e["vals"]) for e in want["pu"]]
    assert [(e["z"], e["compared"], e["n_num"], e["n_den"], [tuple(v) for v in e["num"]], [tuple(v) for v in e["den"]])
            for e in got["z"]] == \
        [(e["z"], e["compared"], e["n_num"], e["n_den"], e["num"], e["den"]) for e in want["z"]]
    gi, wi = got["identities"], want["identities"]
    assert (gi["ran"], gi["n_bad"], gi["rows"]) == (wi["ran"], wi["n_bad"], wi["rows"])
    assert [int(x) for x in gi["value"]] == wi["value"] and [int(x) for x in gi["alpha"]] == wi["alpha"]
    if wi["ran"] and wi["n_bad"]:
        assert gi["failing_terms"] == [ids for ids, _ in want["named"]]


def _no_proof(out):
    assert not os.path.exists(out / "batch_proof.zkin.json") and not os.path.exists(out / "batch_proof.proof.json")


def test_clean_trace(world, tmp_path):
    inst, o, clean = world
    r, out = _run(world, tmp_path, clean, "--audit")
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert r.stdout.splitlines()[0] == "trace audit: 2^8 = 256 rows, 2 plookup(s), %d grand product(s): clean" % \
        len(inst.z_ctx)
    _same(json.loads((out / "trace_audit.json").read_text()), _reference(world, tmp_path, clean))
    _no_proof(out)


def test_every_layer_at_once_with_contexts(world, tmp_path):
    inst, o, clean = world
    v = ac.absent_value(inst, o)
    bad = ac.plant(inst, clean, identity_rows=[5], perm_cells=[(77, 2)], lookup_cells=[(1, 17, v), (1, 200, v)])
    r, out = _run(world, tmp_path, bad, "--audit")
    assert r.returncode == 3, (r.returncode, r.stdout, r.stderr)
    text = r.stdout
    assert "NOT clean" in text.splitlines()[0]
    assert "Number not included: w=17 plookup_number=1: plookup 1 (puCtx[1]): 2 row(s) of f hold 1 value(s)" in text
    # the driver's products: the two plookups, then peCtx
    assert "grand product 1 is plookup 1 (puCtx[1]); it follows from the misses of plookup 1" in text
    assert "1 value(s) of den unmatched, the first at row 77 (0 in num, 1 in den)" in text
    assert "grand product 2 is permutation check 0 (peCtx[0])" in text
    assert "follows from" not in [l for l in text.splitlines() if "grand product 2 does not close" in l][0]
    assert "constraint check: not run: a plookup missed" in text
    got = json.loads((out / "trace_audit.json").read_text())
    _same(got, _reference(world, tmp_path, bad))
    assert [e["context"] for e in got["pu"]] == ["plookup 1 (puCtx[1])"]
    assert [e["context"] for e in got["z"]] == ["plookup 1 (puCtx[1])", "permutation check 0 (peCtx[0])"]
    _no_proof(out)


def test_identities_and_an_open_product(world, tmp_path):
    inst, o, clean = world
    bad = ac.plant(inst, clean, identity_rows=[5, N - 1], perm_cells=[(77, 2)])
    r, out = _run(world, tmp_path, bad, "--audit")
    assert r.returncode == 3, (r.returncode, r.stdout, r.stderr)
    want = _reference(world, tmp_path, bad)
    _same(json.loads((out / "trace_audit.json").read_text()), want)
    assert want["identities"]["ran"] == 1 and {5, N - 1} <= set(want["identities"]["rows"])
    assert "rows of the trace break the AIR; the first is row %d" % want["identities"]["rows"][0] in r.stdout
    assert "  row 5: failing terms:" in r.stdout
    _no_proof(out)


def test_refused_with_a_sharded_run(world, tmp_path):
    inst, o, clean = world
    r, out = _run(world, tmp_path, clean, "--audit", "--shard", "0/2", "--comm", "host:/zkgpu_audit_refused")
    assert r.returncode == 1 and "--audit is for the single-GPU prover" in r.stderr, (r.returncode, r.stderr)
    assert not os.path.exists(out / "trace_audit.json")
    _no_proof(out)
