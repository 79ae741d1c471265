"""zkgpu_batch_prover on a trace whose permutation check does not close: the
run ends with a non-zero status, the diagnosis and the starkinfo context of
the product in the message, and no proof file; on the unchanged files the zkin
is the oracle's, byte for byte."""
import os
import subprocess

import pytest

from test_starkinfo import DRIVER

pytestmark = pytest.mark.gpu

P = 0xFFFFFFFF00000001
ROW = 77


@pytest.fixture(scope="module")
def proved(oracle):
    from oracle.stark_prover import OracleStark
    from zkgpu.synthetic import SyntheticStark
    inst = SyntheticStark(n_bits=8, t=2, m=1, n_queries=8, n_perms=1)
    o = OracleStark(inst)
    o.witness()
    return inst, o, o.S[0].copy(), o.prove()


def test_clean_commit_file_proves_as_the_oracle(proved, tmp_path):
    import zkgpu.starkinfo as zs
    inst, o, cm1, proof = proved
    cfg = zs.write_inputs(str(tmp_path), inst, o.S[4], o.S[9], o.const_nodes, cm1, o.publics)
    r = subprocess.run([DRIVER, cfg], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "out" / "batch_proof.zkin.json").read_text() == zs.zkin_text(proof, o.publics, inst.n_cm2,
                                                                                     inst.n_cm3)


def test_one_altered_cell_is_named(proved, tmp_path):
    import zkgpu.starkinfo as zs
    inst, o, cm1, _ = proved
    bad = cm1.copy()
    c = inst.perms[0]["cols"][2]
    bad[ROW, c] = (int(bad[ROW, c]) + 1) % P
    cfg = zs.write_inputs(str(tmp_path), inst, o.S[4], o.S[9], o.const_nodes, bad, o.publics)
    r = subprocess.run([DRIVER, cfg], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1, (r.returncode, r.stderr)
    # the driver's products: the two plookups, then peCtx
    assert "calculateZ: grand product 2 does not close" in r.stderr, r.stderr
    assert "1 value(s) of den unmatched, the first at row %d (0 in num, 1 in den)" % ROW in r.stderr, r.stderr
    assert "1 value(s) of num unmatched, the first at row %d (1 in num, 0 in den)" % (ROW + inst.PERM_ROT) in r.stderr
    assert "grand product 2 is permutation check 0 (peCtx[0])" in r.stderr, r.stderr
    assert not os.path.exists(tmp_path / "out" / "batch_proof.zkin.json")
    assert not os.path.exists(tmp_path / "out" / "batch_proof.proof.json")
