"""zkgpu_stark_set_exec + zkgpu_stark_set_cm1_witness (host/starks.cpp): the
recursion STARKs' way in, circom witness -> .exec hand-off -> cm1_n on the GPU.
The trace of each instance is factored into a witness and an .exec image
(zkgpu.exec_file.exec_from_rows); loading it through the hand-off must leave
the prover exactly as set_cm1(rows) does: the oracle's proof bit for bit under
either memory plan, get_cm1() == rows, and an audit that reports what it
reports after set_cm1(rows) and changes nothing: clean for config-4.  The
zkEVM-shaped instance has the zkEVM's shapes, not a satisfiable AIR -- the
audit of its own trace names all 1024 rows as breaking an identity whichever
way the trace was loaded (witness(), set_cm1) -- so there the whole report is
held to set_cm1's, findings included, instead of to "clean".
The refusals: no plan set, an sMap longer than the trace, a sharded handle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KINDS = [False, "zkevm"]
KIND_IDS = ["config4", "zkevm_shaped"]


def _inst(kind):
    import bench
    return bench.stark_instance(10, 1, 100, 16, kind)


@pytest.fixture(scope="module")
def oracle_proofs(oracle):
    from oracle.stark_prover import OracleStark
    out = {}
    for kind in KINDS:
        o = OracleStark(_inst(kind))
        o.witness()
        out[kind] = o.prove()
    return out


@pytest.fixture(scope="module")
def handoffs(zkgpu):
    """per instance: the executor's row-major buffer (a resident prover's
    witness read back), its factoring (witness, image), and the audit's report
    of the trace loaded by set_cm1"""
    from zkgpu.exec_file import exec_from_rows
    from zkgpu.stark import GpuStark, MEM_RESIDENT
    out = {}
    for k, kind in enumerate(KINDS):
        r = GpuStark(_inst(kind), mode=MEM_RESIDENT)
        try:
            r.witness()
            rows = r.get_cm1()
            r.set_cm1(rows)
            report = r.audit()
        finally:
            r.close()
        assert report["clean"] == (0 if kind else 1)
        out[kind] = (rows,) + exec_from_rows(rows, np.random.default_rng(40 + k)) + (report,)
    return out


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_resident_proof_trace_and_audit(zkgpu, oracle_proofs, handoffs, kind):
    from zkgpu.stark import GpuStark, MEM_RESIDENT
    rows, witness, image, report = handoffs[kind]
    g = GpuStark(_inst(kind), mode=MEM_RESIDENT)
    try:
        g.set_exec(image, witness.size)
        g.set_cm1_async(np.zeros_like(rows))  # superseded, as set_cm1 supersedes it
        g.set_cm1_witness(witness)
        assert list(g.timers()) == ["ZKGPU_EXEC_COMMIT"]
        assert np.array_equal(g.get_cm1(), rows)
        p1 = g.prove()
        assert p1 == oracle_proofs[kind]
        assert list(g.timers())[-1] == "ZKGPU_EXEC_COMMIT"
        assert g.audit() == report
        assert g.prove() == p1
        assert "ZKGPU_EXEC_COMMIT" not in g.timers()  # that proof loaded nothing
        g.set_cm1(np.zeros_like(rows))
        g.set_cm1_witness(witness)  # over another trace: every cell is written
        assert g.prove() == p1
    finally:
        g.close()


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_lean_proof_equals_oracle(zkgpu, oracle_proofs, handoffs, kind):
    from zkgpu import ZkgpuError
    from zkgpu.stark import GpuStark, MEM_LEAN
    rows, witness, image, report = handoffs[kind]
    g = GpuStark(_inst(kind), mode=MEM_LEAN)
    try:
        assert g.memory_mode() == "lean"
        g.set_exec(image, witness.size)
        g.set_cm1_witness(witness)
        assert g.audit() == report
        assert g.prove() == oracle_proofs[kind]
        with pytest.raises(ZkgpuError, match="consumed the trace"):
            g.prove_raw()
        g.set_cm1_witness(witness)  # loads the next proof's trace, as set_cm1 does
        assert g.prove() == oracle_proofs[kind]
    finally:
        g.close()


def test_refusals(zkgpu, handoffs):
    import os
    from zkgpu import ZkgpuError
    from zkgpu.exec_file import make_image, split_image
    from zkgpu.stark import GpuStark, MEM_RESIDENT, ShmComm
    rows, witness, image, _ = handoffs[False]
    n, n_cols = rows.shape
    g = GpuStark(_inst(False), mode=MEM_RESIDENT)
    try:
        with pytest.raises(ZkgpuError, match="no .exec plan is set; call set_exec first"):
            g.set_cm1_witness(witness)
        adds, smap = split_image(image, n_cols)
        longer = make_image(adds, np.concatenate([smap, smap[:1]]))
        with pytest.raises(ZkgpuError, match="the sMap has %d rows, the trace %d" % (n + 1, n)):
            g.set_exec(longer, witness.size)
        with pytest.raises(ZkgpuError, match="the image has %d words, not" % (image.size - 1)):
            g.set_exec(image[:-1], witness.size)
        with pytest.raises(ZkgpuError, match="no .exec plan is set"):  # the refused plans left none
            g.set_cm1_witness(witness)
        g.witness()
        g.prove_raw()  # the refused calls changed nothing
    finally:
        g.close()
    comm = ShmComm("/zkgpu_exw_%d" % os.getpid(), 1, 0, capacity=1 << 20)
    try:
        s = GpuStark(_inst(False), comm=comm)
        try:
            with pytest.raises(ZkgpuError, match="set_exec is single-GPU only"):
                s.set_exec(image, witness.size)
            with pytest.raises(ZkgpuError, match="set_cm1_witness is single-GPU only"):
                s.set_cm1_witness(witness)
        finally:
            s.close()
    finally:
        comm.close()
