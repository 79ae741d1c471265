"""The ordered list of stage timers of one proof (GpuStark.timers(): a dict
in the order the library reported them), single GPU and row-sharded.

Starks::prove_body (host/starks.cpp) is the one protocol schedule of both
provers; the row-sharded prover (host/sharded_starks.hpp) overrides the steps
that differ.  The lists below are the timer names of the two schedules the
provers had while each kept its own: a step moved to another place of the
schedule, or a timer renamed, changes a list.  Every case also compares the
proof with the oracle's, so a reordered step cannot pass on its names alone."""
import pytest

from test_gpu_sharded_cpp import _assert_same, _free_port, _inst, _oracle_json, _worker

pytestmark = pytest.mark.gpu

RESIDENT = [
    "STARK_STEP_1_LDE", "STARK_STEP_1_MERKLETREE",
    "STARK_STEP_2_CALCULATE_EXPS", "STARK_STEP_2_CALCULATEH1H2", "STARK_STEP_2_LDE", "STARK_STEP_2_MERKLETREE",
    "STARK_STEP_3_CALCULATE_EXPS", "STARK_STEP_3_CALCULATE_Z", "STARK_STEP_3_CALCULATE_EXPS_2", "STARK_STEP_3_LDE",
    "STARK_STEP_3_MERKLETREE",
    "STARK_STEP_4_CALCULATE_EXPS_2NS", "STARK_STEP_4_CALCULATE_EXPS_2NS_INTT_NTT", "STARK_STEP_4_MERKLETREE",
    "STARK_STEP_5_LEv_LpEv", "STARK_STEP_5_EVMAP", "STARK_STEP_5_XDIVXSUB", "STARK_STEP_5_CALCULATE_EXPS",
    "STARK_STEP_FRI_FOLDS", "STARK_STEP_FRI_QUERIES", "STARK_TOTAL",
]
# the lean plan extends cm1 again before the quotient program
LEAN = [
    "STARK_STEP_1_LDE", "STARK_STEP_1_MERKLETREE",
    "STARK_STEP_2_CALCULATE_EXPS", "STARK_STEP_2_CALCULATEH1H2", "STARK_STEP_2_LDE", "STARK_STEP_2_MERKLETREE",
    "STARK_STEP_3_CALCULATE_EXPS", "STARK_STEP_3_CALCULATE_Z", "STARK_STEP_3_CALCULATE_EXPS_2", "STARK_STEP_3_LDE",
    "STARK_STEP_3_MERKLETREE",
    "STARK_STEP_4_CM1_LDE", "STARK_STEP_4_CALCULATE_EXPS_2NS", "STARK_STEP_4_CALCULATE_EXPS_2NS_INTT_NTT",
    "STARK_STEP_4_MERKLETREE",
    "STARK_STEP_5_LEv_LpEv", "STARK_STEP_5_EVMAP", "STARK_STEP_5_XDIVXSUB", "STARK_STEP_5_CALCULATE_EXPS",
    "STARK_STEP_FRI_FOLDS", "STARK_STEP_FRI_QUERIES", "STARK_TOTAL",
]
# the streamed stage 1 is one timer (load, LDE and leaf sponge overlap)
FROM_ROWS = [
    "STARK_STEP_1_STREAM",
    "STARK_STEP_2_CALCULATE_EXPS", "STARK_STEP_2_CALCULATEH1H2", "STARK_STEP_2_LDE", "STARK_STEP_2_MERKLETREE",
    "STARK_STEP_3_CALCULATE_EXPS", "STARK_STEP_3_CALCULATE_Z", "STARK_STEP_3_CALCULATE_EXPS_2", "STARK_STEP_3_LDE",
    "STARK_STEP_3_MERKLETREE",
    "STARK_STEP_4_CALCULATE_EXPS_2NS", "STARK_STEP_4_CALCULATE_EXPS_2NS_INTT_NTT", "STARK_STEP_4_MERKLETREE",
    "STARK_STEP_5_LEv_LpEv", "STARK_STEP_5_EVMAP", "STARK_STEP_5_XDIVXSUB", "STARK_STEP_5_CALCULATE_EXPS",
    "STARK_STEP_FRI_FOLDS", "STARK_STEP_FRI_QUERIES", "STARK_TOTAL",
]
# one rank: the LDE goes straight into the row block, no exchange and no counts
WORLD1 = [
    "STARK_STEP_1_LDE", "STARK_STEP_1_MERKLETREE",
    "STARK_STEP_2_CALCULATE_EXPS", "STARK_STEP_2_CALCULATEH1H2", "STARK_STEP_2_LDE", "STARK_STEP_2_MERKLETREE",
    "STARK_STEP_3_CALCULATE_EXPS", "STARK_STEP_3_CALCULATE_Z", "STARK_STEP_3_CALCULATE_EXPS_2", "STARK_STEP_3_LDE",
    "STARK_STEP_3_MERKLETREE",
    "STARK_STEP_4_CALCULATE_EXPS_2NS", "STARK_STEP_4_CALCULATE_EXPS_2NS_INTT_NTT", "STARK_STEP_4_MERKLETREE",
    "STARK_STEP_5_LEv_LpEv", "STARK_STEP_5_EVMAP", "STARK_STEP_5_XDIVXSUB", "STARK_STEP_5_CALCULATE_EXPS",
    "STARK_STEP_FRI_FOLDS", "STARK_STEP_FRI_QUERIES", "STARK_TOTAL",
]
# every commit: rows -> column shares, LDE, columns -> row blocks, subtree
WORLD2 = [
    "STARK_STEP_1_EXCHANGE_T", "STARK_STEP_1_LDE", "STARK_STEP_1_EXCHANGE", "STARK_STEP_1_MERKLETREE",
    "STARK_STEP_2_CALCULATE_EXPS", "STARK_STEP_2_CALCULATEH1H2",
    "STARK_STEP_2_EXCHANGE_T", "STARK_STEP_2_LDE", "STARK_STEP_2_EXCHANGE", "STARK_STEP_2_MERKLETREE",
    "STARK_STEP_3_CALCULATE_EXPS", "STARK_STEP_3_CALCULATE_Z", "STARK_STEP_3_CALCULATE_EXPS_2",
    "STARK_STEP_3_EXCHANGE_T", "STARK_STEP_3_LDE", "STARK_STEP_3_EXCHANGE", "STARK_STEP_3_MERKLETREE",
    "STARK_STEP_4_CALCULATE_EXPS_2NS", "STARK_STEP_4_CALCULATE_EXPS_2NS_INTT_NTT", "STARK_STEP_4_MERKLETREE",
    "STARK_STEP_5_LEv_LpEv", "STARK_STEP_5_EVMAP", "STARK_STEP_5_XDIVXSUB", "STARK_STEP_5_CALCULATE_EXPS",
    "STARK_STEP_FRI_FOLDS", "STARK_STEP_FRI_QUERIES", "STARK_TOTAL",
    "COUNT_COMM_MAX_OPS", "COUNT_COMM_EXCHANGE_MS", "COUNT_COMM_LARGEST_EXCHANGE_MS", "COUNT_COMM_WORLD",
    "COUNT_COMM_EXCHANGES", "COUNT_COMM_BYTES_SENT", "COUNT_COMM_MAX_BYTES_SENT",
]


@pytest.fixture(scope="module")
def oracle_proofs(oracle):
    return {k: _oracle_json(_inst(k)) for k in ("lookups", "blowup4")}


def test_single_gpu_resident(zkgpu, oracle_proofs):
    from zkgpu.stark import GpuStark, MEM_RESIDENT
    g = GpuStark(_inst("lookups"), mode=MEM_RESIDENT)
    try:
        g.witness()
        _assert_same(g.prove(), oracle_proofs["lookups"])
        assert list(g.timers()) == RESIDENT
    finally:
        g.close()


def test_single_gpu_lean(zkgpu, oracle_proofs):
    from zkgpu.stark import GpuStark, MEM_LEAN
    g = GpuStark(_inst("lookups"), mode=MEM_LEAN)
    try:
        assert g.memory_mode() == "lean"
        g.witness()
        _assert_same(g.prove(), oracle_proofs["lookups"])
        assert list(g.timers()) == LEAN
    finally:
        g.close()


def test_single_gpu_prove_from_rows(zkgpu, oracle_proofs):
    from oracle.stark_prover import OracleStark
    from zkgpu.stark import GpuStark, MEM_RESIDENT
    o = OracleStark(_inst("lookups"))
    o.witness()
    g = GpuStark(_inst("lookups"), mode=MEM_RESIDENT)
    try:
        _assert_same(g.prove_from_rows(o.S[0]), oracle_proofs["lookups"])
        assert list(g.timers()) == FROM_ROWS
    finally:
        g.close()


def test_sharded_world1(zkgpu, oracle_proofs):
    from zkgpu.stark import EXCHANGE, Comm, GpuStark

    class One:
        c = Comm(0, 1, None, EXCHANGE())

    g = GpuStark(_inst("lookups"), comm=One())
    try:
        g.witness()
        _assert_same(g.prove(), oracle_proofs["lookups"])
        assert list(g.timers()) == WORLD1
    finally:
        g.close()


@pytest.mark.parametrize("name", ["lookups", "blowup4"])
def test_sharded_world2(oracle_proofs, name):
    """two processes on the one GPU over the shared-memory communicator;
    blowup4 (a halo of 4 rows, the quotient split over its column owners):
    the smallest shape whose stage-4 / stage-5 row-block offsets differ from
    zero on rank 1"""
    import multiprocessing as mp
    import uuid
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    shm = "/zkgpu_t_%s" % uuid.uuid4().hex[:12]
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, name, shm)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = [q.get(timeout=240) for _ in range(2)]
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    errs = [e for *_, e in res if e]
    assert not errs, errs[0]
    for _, proof, timers, _ in res:
        _assert_same(proof, oracle_proofs[name])
        assert list(timers) == WORLD2
