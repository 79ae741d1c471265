"""zkgpu_batch_prover --circuit <prefix> --witness <file>: the driver reads
the circuit's files under the reference's key names (config.cpp:243-259) and
loads the committed trace from a circom witness through <prefix>Exec on the GPU
(zkgpu_stark_set_exec + zkgpu_stark_set_cm1_witness).  Its
batch_proof.zkin.json equals, byte for byte, the one the driver writes from the
equivalent <prefix>CmPols file under the same prefix (and the oracle's); the
flag conflicts are refused."""
import json
import subprocess

import numpy as np
import pytest

from test_starkinfo import DRIVER

pytestmark = pytest.mark.gpu


def test_witness_gives_the_same_proof_files_as_the_commit_file(oracle, tmp_path):
    import zkgpu.starkinfo as zs
    from oracle.stark_prover import OracleStark
    from zkgpu.exec_file import exec_from_rows
    from zkgpu.synthetic import SyntheticStark
    inst = SyntheticStark(n_bits=9, blowup_bits=2, t=3, m=1, n_lookups=1, q_deg=4, n_queries=12)
    o = OracleStark(inst)
    o.witness()
    proof = o.prove()
    base = json.load(open(zs.write_inputs(str(tmp_path), inst, o.S[4], o.S[9], o.const_nodes, o.S[0], o.publics)))
    witness, image = exec_from_rows(o.S[0], np.random.default_rng(3))
    (tmp_path / "recursive1.exec").write_bytes(image.tobytes())
    (tmp_path / "witness.bin").write_bytes(witness.tobytes())

    def config(name, out, with_commit):
        cfg = {k.replace("zkevm", "recursive1", 1): v for k, v in base.items() if k.startswith("zkevm")}
        if not with_commit:
            del cfg["recursive1CmPols"]  # the witness run never opens it
        cfg.update(recursive1Exec=str(tmp_path / "recursive1.exec"), zkgpuPublics=base["zkgpuPublics"],
                   outputPath=str(tmp_path / out))
        (tmp_path / name).write_text(json.dumps(cfg, indent=4))
        return str(tmp_path / name)

    c_rows, c_wit = config("rows.json", "out_rows", True), config("wit.json", "out_wit", False)
    wit = ["--witness", str(tmp_path / "witness.bin")]
    r = subprocess.run([DRIVER, "--circuit", "recursive1", c_rows], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([DRIVER, "--circuit", "recursive1"] + wit + [c_wit], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = (tmp_path / "out_wit" / "batch_proof.zkin.json").read_bytes()
    assert got == (tmp_path / "out_rows" / "batch_proof.zkin.json").read_bytes()
    assert got.decode() == zs.zkin_text(proof, o.publics, inst.n_cm2, inst.n_cm3)
    assert (tmp_path / "out_wit" / "batch_proof.proof.json").read_bytes() == \
        (tmp_path / "out_rows" / "batch_proof.proof.json").read_bytes()

    # --check-trace and --audit take the trace from the witness too
    r = subprocess.run([DRIVER, "--circuit", "recursive1", "--check-trace"] + wit + [c_wit], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "out_wit" / "batch_proof.zkin.json").read_bytes() == got
    r = subprocess.run([DRIVER, "--circuit", "recursive1", "--audit"] + wit + [c_wit], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert json.loads((tmp_path / "out_wit" / "trace_audit.json").read_text())["clean"] == 1

    # without --circuit the zkevm keys are asked for; a witness of another length is the planner's refusal
    r = subprocess.run([DRIVER] + wit + [c_wit], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "zkevmStarkInfo" in r.stderr, r.stderr
    (tmp_path / "short.bin").write_bytes(witness[:-1].tobytes())
    r = subprocess.run([DRIVER, "--circuit", "recursive1", "--witness", str(tmp_path / "short.bin"), c_wit],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "set_exec: exec_plan: " in r.stderr, r.stderr

    # flag conflicts
    r = subprocess.run([DRIVER, "--circuit", "recursive1", "--stream-trace"] + wit + [c_wit], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 1 and "--witness loads the trace on the GPU: not with --stream-trace" in r.stderr, r.stderr
    r = subprocess.run([DRIVER, "--circuit", "recursive1", "--shard", "0/2", "--comm", "host:/zkgpu_none"] + wit + [c_wit],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--witness is for the single-GPU prover" in r.stderr, r.stderr
