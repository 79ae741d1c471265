"""zkgpu_batch_prover --check-trace: the constraint check in its STOP mode from
the reference's input files.  A commit file with one cell changed ends the
run with a non-zero status, the failing row in the message and no proof
files; on the unchanged files the zkin is the oracle's, byte for byte."""
import os
import subprocess

import pytest

from test_starkinfo import DRIVER

pytestmark = pytest.mark.gpu

P = 0xFFFFFFFF00000001
ROW = 77


@pytest.fixture(scope="module")
def proved(oracle):
    """the smallest instance of tests/test_gpu_batch_prover.py"""
    from oracle.stark_prover import OracleStark
    from zkgpu.synthetic import SyntheticStark
    inst = SyntheticStark(n_bits=8, t=2, m=1, n_queries=8)
    o = OracleStark(inst)
    o.witness()
    cm1 = o.S[0].copy()
    return inst, o, cm1, o.prove()


def test_check_trace_stops_on_a_broken_row(proved, tmp_path):
    import zkgpu.starkinfo as zs
    inst, o, cm1, _ = proved
    bad = cm1.copy()
    bad[ROW, 2] = (int(bad[ROW, 2]) + 1) % P  # a2 of triple 0: row ROW breaks a0 * a1 * K + a0 = a2
    cfg = zs.write_inputs(str(tmp_path), inst, o.S[4], o.S[9], o.const_nodes, bad, o.publics)
    r = subprocess.run([DRIVER, "--check-trace", cfg], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert "constraint check: 1 of the 2^8 = 256 rows" in r.stderr and "the first is row %d " % ROW in r.stderr, r.stderr
    assert not os.path.exists(tmp_path / "out" / "batch_proof.zkin.json")
    assert not os.path.exists(tmp_path / "out" / "batch_proof.proof.json")


def test_check_trace_leaves_a_clean_proof_as_it_is(proved, tmp_path):
    import zkgpu.starkinfo as zs
    inst, o, cm1, proof = proved
    cfg = zs.write_inputs(str(tmp_path), inst, o.S[4], o.S[9], o.const_nodes, cm1, o.publics)
    r = subprocess.run([DRIVER, "--check-trace", cfg], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "out" / "batch_proof.zkin.json").read_text() == zs.zkin_text(proof, o.publics, inst.n_cm2,
                                                                                     inst.n_cm3)


def test_check_trace_is_refused_on_a_sharded_run(tmp_path):
    r = subprocess.run([DRIVER, "--check-trace", "--shard", "0/2", "--comm", "host:/zkgpu_none", str(tmp_path / "c.json")],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--check-trace is for the single-GPU prover" in r.stderr, r.stderr
