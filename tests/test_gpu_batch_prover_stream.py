"""zkgpu_batch_prover --stream-trace: the driver proves through
zkgpu_stark_prove_from_rows (the trace file's rows stay in host memory and
cross PCIe under stage 1) and writes the same files as the default path; the
flag is refused with a sharded prover."""
import subprocess

import pytest

from test_starkinfo import DRIVER

pytestmark = pytest.mark.gpu


def test_stream_trace_gives_the_same_proof_files(oracle, tmp_path):
    import zkgpu.starkinfo as zs
    from oracle.stark_prover import OracleStark
    from zkgpu.synthetic import SyntheticStark
    inst = SyntheticStark(n_bits=9, blowup_bits=2, t=3, m=1, n_lookups=1, q_deg=4, n_queries=12)
    o = OracleStark(inst)
    o.witness()
    proof = o.prove()
    cfg = zs.write_inputs(str(tmp_path), inst, o.S[4], o.S[9], o.const_nodes, o.S[0], o.publics)
    r = subprocess.run([DRIVER, "--stream-trace", cfg], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = (tmp_path / "out" / "batch_proof.zkin.json").read_text()
    assert got == zs.zkin_text(proof, o.publics, inst.n_cm2, inst.n_cm3)
    r = subprocess.run([DRIVER, "--stream-trace", "--shard", "0/1", "--comm", "host:/zkgpu_none", cfg],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--stream-trace is for the single-GPU prover" in r.stderr, r.stderr
