"""What a row-sharded prover answers to the single-GPU entry points
(include/zkgpu_stark.h): the thirteen calls it refuses, each with its whole
message, and the five readers it does not refuse, which return what a prover
that never ran a diagnostic returns.  On a world-1 shared-memory prover of the
constraint check's smallest instance; nothing but the prover's creation touches
the device."""
import ctypes
import uuid

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REFUSED = {
    "get_cm1": "stark (sharded): get_cm1 is single-GPU only",
    "probe_set": "stark (sharded): probe_set is single-GPU only (the sampled rows live on other ranks)",
    "check_set": "stark (sharded): check_set is single-GPU only (the n-domain sections live in row blocks on the "
                 "ranks)",
    "z_diag": "stark (sharded): z_diag: single-GPU provers only (a rank holds a row block of num and den)",
    "audit": "stark (sharded): audit: single-GPU provers only (a rank holds a row block of the n-domain sections)",
    "audit_format": "stark (sharded): audit_format: single-GPU provers only",
    "conn_set": "stark (sharded): conn_set: single-GPU provers only (as the audit)",
    "conn_check": "stark (sharded): conn_check: single-GPU provers only (a rank holds a row block of the n-domain "
                  "sections)",
    "audit_conn": "stark (sharded): audit_conn: single-GPU provers only",
    "check_names_set": "stark (sharded): check_names_set is single-GPU only (as check_set)",
    "prove_from_rows": "stark (sharded): prove_from_rows is single-GPU only (each rank loads its rows: set_cm1 / "
                       "set_cm1_async, then prove)",
    "set_exec": "stark (sharded): set_exec is single-GPU only (the recursion circuits' traces fit one device)",
    "set_cm1_witness": "stark (sharded): set_cm1_witness is single-GPU only (the recursion circuits' traces fit one "
                       "device)",
}


@pytest.fixture(scope="module")
def sharded(zkgpu):
    import bench
    from zkgpu.stark import GpuStark, ShmComm
    inst = bench.stark_instance(10, 1, 100, 16, False)
    comm = ShmComm("/zkgpu_ref_%s" % uuid.uuid4().hex[:12], 1, 0, capacity=1 << 20)
    try:
        g = GpuStark(inst, comm=comm)
        try:
            yield g, inst
        finally:
            g.close()
    finally:
        comm.close()


def _calls(g, inst):
    rows = np.zeros((1 << inst.n_bits, inst.n_cm1), np.uint64)
    words = np.zeros(8, np.uint64)
    return {
        "get_cm1": g.get_cm1,
        "probe_set": lambda: g.probe_set([0], [0]),
        "check_set": lambda: g.check_set(1),
        "z_diag": g.z_diag,
        "audit": g.audit,
        "audit_format": g.audit_text,
        "conn_set": lambda: g.conn_set(0, [0], [0]),
        "conn_check": lambda: g.conn_check(0),
        "audit_conn": lambda: g.audit_conn(0),
        "check_names_set": lambda: g.check_names_set(True),
        "prove_from_rows": lambda: g.prove_from_rows_raw(rows),
        "set_exec": lambda: g.set_exec(words, 8),
        "set_cm1_witness": lambda: g.set_cm1_witness(words),
    }


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refused_with_its_whole_message(sharded, name):
    from zkgpu import ZkgpuError
    g, inst = sharded
    with pytest.raises(ZkgpuError) as e:
        _calls(g, inst)[name]()
    assert str(e.value).split(" failed: ", 1)[1] == REFUSED[name]


def test_refused_with_null_arguments_too(sharded):
    """the refusal comes before any look at the arguments"""
    from zkgpu.stark import slib
    g, _ = sharded
    lib = slib()
    for rc in (lib.zkgpu_stark_get_cm1(g.h, None), lib.zkgpu_stark_z_diag(g.h, None),
               lib.zkgpu_stark_audit(g.h, 0xFF, None), lib.zkgpu_stark_conn_check(g.h, 1 << 20, None),
               lib.zkgpu_stark_prove_from_rows(g.h, None, 0, None), lib.zkgpu_stark_set_exec(g.h, None, 0, 0)):
        assert rc == -1
        assert lib.zkgpu_stark_last_error().decode().startswith("stark (sharded): ")


def test_readers_answer_as_a_prover_that_ran_no_diagnostic(sharded):
    from zkgpu import ZkgpuError
    from zkgpu.stark import slib
    g, _ = sharded
    assert g.check_result() == {"ran": 0, "n_bad": 0, "rows": [0] * 16, "value": [0, 0, 0], "alpha": [0, 0, 0]}
    assert g.probe_size() == (0, 0)
    with pytest.raises(ZkgpuError) as e:
        g.probe_read_raw()
    assert str(e.value).split(" failed: ", 1)[1] == ("probe_read: no probe to read: none was set (probe_set) before "
                                                     "the last proof, or that proof failed")
    n = ctypes.c_uint32(7)
    assert slib().zkgpu_stark_check_terms(g.h, None, 0, ctypes.byref(n)) == -1 and n.value == 0
    assert slib().zkgpu_stark_last_error().decode() == "check_terms: naming has not been set on this prover"
    n = ctypes.c_uint32(7)
    assert slib().zkgpu_stark_check_named(g.h, 0, None, None, 0, ctypes.byref(n)) == -1 and n.value == 0
    assert slib().zkgpu_stark_last_error().decode() == "check_named: the last proof ran no check with naming on"
