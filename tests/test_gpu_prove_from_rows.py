"""zkgpu_stark_prove_from_rows (host/starks.cpp commit_cm1_stream): one proof
of the executor's host buffer, the trace loaded in column batches under stage 1
(load -> LDE -> chunked leaf sponge per batch).  Under either memory plan the
proof must equal set_cm1(rows) + prove() -- the oracle's proof -- bit for bit,
whatever the batch width and, under the lean plan, wherever the kept columns
split the section; a load that fails mid-stream must fail the call and leave
the prover refusing prove() until a whole trace is loaded again."""
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
def traces(zkgpu):
    """the executor's row-major buffer per instance: a resident prover's
    witness read back"""
    from zkgpu.stark import GpuStark, MEM_RESIDENT
    out = {}
    for kind in KINDS:
        r = GpuStark(_inst(kind), mode=MEM_RESIDENT)
        try:
            r.witness()
            out[kind] = r.get_cm1()
        finally:
            r.close()
    return out


def _env(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, value)


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("keep", ["0", "45", "100000"], ids=["keep0", "keep_part", "keep_all"])
@pytest.mark.parametrize("cols", ["8", "24", None], ids=["cols8", "cols24", "cols_default"])
def test_lean_proof_equals_oracle(zkgpu, oracle_proofs, traces, monkeypatch, kind, keep, cols):
    from zkgpu import ZkgpuError
    from zkgpu.stark import GpuStark, MEM_LEAN
    _env(monkeypatch, "ZKGPU_STREAM_COLS", cols)
    monkeypatch.delenv("ZKGPU_STREAM_FAIL_BATCH", raising=False)
    monkeypatch.setenv("ZKGPU_LEAN_KEEP_COLS", keep)
    rows = traces[kind]
    g = GpuStark(_inst(kind), mode=MEM_LEAN)
    try:
        assert g.memory_mode() == "lean"
        p1 = g.prove_from_rows(rows)
        assert p1 == oracle_proofs[kind]
        assert "STARK_STEP_1_STREAM" in g.timers() and "STARK_STEP_1_LDE" not in g.timers()
        with pytest.raises(ZkgpuError, match="consumed the trace"):
            g.prove_raw()
        assert g.prove_from_rows(rows) == p1
    finally:
        g.close()


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("cols", ["8", None], ids=["cols8", "cols_default"])
def test_resident_proof_equals_oracle(zkgpu, oracle_proofs, traces, monkeypatch, kind, cols):
    from zkgpu.stark import GpuStark, MEM_RESIDENT
    _env(monkeypatch, "ZKGPU_STREAM_COLS", cols)
    monkeypatch.delenv("ZKGPU_STREAM_FAIL_BATCH", raising=False)
    rows = traces[kind]
    g = GpuStark(_inst(kind), mode=MEM_RESIDENT)
    try:
        p1 = g.prove_from_rows(rows, register_host=(cols is None))
        assert p1 == oracle_proofs[kind]
        assert np.array_equal(g.get_cm1(), rows)
        assert g.prove() == p1  # the resident plan keeps the trace
    finally:
        g.close()


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("mode", ["lean", "resident"])
def test_injected_load_failure(zkgpu, oracle_proofs, traces, monkeypatch, kind, mode):
    """the loader fails before queuing batch 1 (a host-side error return):
    the call fails with its message, prove() is refused, and set_cm1 + prove
    then gives the right proof"""
    from zkgpu import ZkgpuError
    from zkgpu.stark import GpuStark, MEM_LEAN, MEM_RESIDENT
    monkeypatch.setenv("ZKGPU_STREAM_COLS", "8")
    monkeypatch.setenv("ZKGPU_STREAM_FAIL_BATCH", "1")
    rows = traces[kind]
    g = GpuStark(_inst(kind), mode=MEM_LEAN if mode == "lean" else MEM_RESIDENT)
    try:
        if mode == "resident":
            g.witness()  # a whole trace is loaded: the failed stream must invalidate it
        with pytest.raises(ZkgpuError, match="injected failure before batch 1"):
            g.prove_from_rows_raw(rows)
        with pytest.raises(ZkgpuError, match="failed part-way"):
            g.prove_raw()
        monkeypatch.delenv("ZKGPU_STREAM_FAIL_BATCH")
        g.set_cm1(rows)
        assert g.prove() == oracle_proofs[kind]
        if mode == "lean":
            assert g.prove_from_rows(rows) == oracle_proofs[kind]
    finally:
        g.close()


def test_null_rows_is_an_argument_error(zkgpu):
    import ctypes
    from zkgpu import ZkgpuError
    from zkgpu.stark import GpuStark, MEM_RESIDENT, slib
    g = GpuStark(_inst(False), mode=MEM_RESIDENT)
    try:
        buf = np.zeros(slib().zkgpu_stark_proof_len(g.h), np.uint64)
        assert slib().zkgpu_stark_prove_from_rows(g.h, None, 0, buf.ctypes.data) != 0
        assert b"null argument" in slib().zkgpu_stark_last_error()
        g.witness()
        g.prove_raw()  # the refused call changed nothing
    finally:
        g.close()


def test_pending_background_load_is_dropped(zkgpu, oracle_proofs, traces):
    """resident plan: a set_cm1_async trace still pending is dropped by
    prove_from_rows, as by set_cm1 -- the next prove() runs on `rows`"""
    from zkgpu.stark import GpuStark, MEM_RESIDENT
    rows = traces[False]
    g = GpuStark(_inst(False), mode=MEM_RESIDENT)
    try:
        g.set_cm1_async(np.zeros_like(rows))
        assert g.prove_from_rows(rows) == oracle_proofs[False]
        assert g.prove() == oracle_proofs[False]
    finally:
        g.close()


def test_sharded_prover_refuses(zkgpu, traces):
    """a row-sharded prover (world 1, host shared-memory communicator)
    refuses the call with a clear message"""
    import os
    from zkgpu import ZkgpuError
    from zkgpu.stark import GpuStark, ShmComm
    comm = ShmComm("/zkgpu_pfr_%d" % os.getpid(), 1, 0, capacity=1 << 20)
    try:
        g = GpuStark(_inst(False), comm=comm)
        try:
            with pytest.raises(ZkgpuError, match="prove_from_rows is single-GPU only"):
                g.prove_from_rows_raw(traces[False])
        finally:
            g.close()
    finally:
        comm.close()
