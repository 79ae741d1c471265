"""zkgpu_zxp_to_n_domain (csrc/zxp_n_domain.cpp): a quotient program re-targeted
to the trace domain.  The library's rewrite equals the restatement of the rules
in tests/check_cases.py on the quotient programs of the instances the suite
proves; every rule refuses its own defect with its own message; and, on the
CPU oracle alone, the restated program is zero on every row of a clean trace
(which pins the row shifts, the wrap at row N - 1 and the ZI removal) and
nonzero on exactly the corrupted rows.  CPU only."""
import os
import sys

import numpy as np
import pytest

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__))]
import check_cases as cc  # noqa: E402
from check_cases import (ADD, CHAL, COL, COL3, COPY, EVAL, LIT, MUL, PUB, SUB, TMP1, TMP3, X, XDIV, XDIVW, ZI,  # noqa: E402
                         SEC_CM1_2NS, SEC_CM1_N, SEC_CM2_2NS, SEC_CM3_2NS, SEC_CM4_2NS, SEC_CONST_2NS, SEC_F_2NS,
                         SEC_Q_2NS, SEC_TMP_N)

P = cc.P
ERR_ARG = -2


def instance(spec):
    import bench
    return bench.stark_instance(*spec)


INSTANCES = {"config4": (10, 1, 100, 16), "blowup2": (10, 2, 100, 16), "fork9": (10, 1, 100, 16, True),
             "zkevm": (10, 1, 100, 16, "zkevm")}


@pytest.mark.parametrize("name", sorted(INSTANCES))
def test_rewrite_equals_the_restatement(name):
    import zkgpu
    inst = instance(INSTANCES[name])
    ins, opn = inst.programs["step42ns"].arrays()
    eb = inst.n_bits_ext - inst.n_bits
    want = cc.to_n_domain(ins, opn, eb)
    got = zkgpu.zxp_to_n_domain(ins, opn, eb)
    assert got.shape == want.shape and np.array_equal(got, want)
    # the rewrite changed something, and left no operand of the extended domain but q
    assert not np.array_equal(got, opn)
    cols = got[(got[:, 0] == COL) | (got[:, 0] == COL3)]
    assert set(cols[:, 1].tolist()) <= {0, 1, 2, 4, SEC_Q_2NS}
    assert not (got[:, 0] == ZI).any()


# ---- refusals: one defect at a time in a small valid program (extend_bits 1)
def base():
    opn = [(TMP1, 0, 0, 0), (TMP3, 0, 0, 0), (COL, SEC_CM1_2NS, 0, 0), (COL, SEC_CM1_2NS, 1, 2),
           (COL3, SEC_CM2_2NS, 0, -2), (COL3, SEC_CM3_2NS, 0, 4), (COL, SEC_CONST_2NS, 0, 0), (LIT, 5, 0, 0),
           (CHAL, 4, 0, 0), (PUB, 0, 0, 0), (X, 0, 0, 0), (ZI, 0, 0, 0), (COL3, SEC_Q_2NS, 0, 0)]
    ins = [(MUL, 0, 2, 3), (ADD, 0, 0, 6), (SUB, 0, 0, 7), (MUL, 0, 0, 10), (ADD, 0, 0, 9), (MUL, 1, 4, 8),
           (ADD, 1, 1, 5), (ADD, 1, 1, 0), (MUL, 12, 1, 11)]
    return np.array(ins, np.int64), np.array(opn, np.int64)


def _opn(k, col, v):
    def f(ins, opn):
        opn[k, col] = v
    return f


def _ins(k, col, v):
    def f(ins, opn):
        ins[k, col] = v
    return f


def _zi_into_tmp(ins, opn):
    ins[7] = (MUL, 1, 1, 11)  # tmp3 = tmp3 * ZI: ZI feeds a temporary


def _no_zi(ins, opn):
    ins[8] = (COPY, 12, 1, 0)


def _read_q(ins, opn):
    ins[7] = (ADD, 1, 1, 12)


def _store_cm1(ins, opn):
    ins[4] = (COPY, 2, 0, 0)


REFUSED = {
    "shift_1_at_extend_bits_1": (_opn(3, 3, 1), "zxp_to_n_domain: operand 3: row shift 1 is no multiple of 2"),
    "negative_shift_odd": (_opn(4, 3, -3), "zxp_to_n_domain: operand 4: row shift -3 is no multiple of 2"),
    "zi_feeds_a_temporary": (_zi_into_tmp, "zxp_to_n_domain: instruction 7 uses ZI other than as a factor of a "
                                           "product stored to SEC_Q_2NS"),
    "zi_added": (_ins(8, 0, ADD), "zxp_to_n_domain: instruction 8 uses ZI other than as a factor of a product stored "
                                  "to SEC_Q_2NS"),
    "no_zi": (_no_zi, "zxp_to_n_domain: no product by ZI is stored to SEC_Q_2NS: not a quotient program"),
    "read_of_q": (_read_q, "zxp_to_n_domain: operand 12 reads SEC_Q_2NS"),
    "q_shifted_store": (_opn(12, 3, 2), "zxp_to_n_domain: operand 12 stores to SEC_Q_2NS at row shift 2"),
    "store_to_cm1": (_store_cm1, "zxp_to_n_domain: operand 2 stores to section 5"),
    "eval": (_opn(9, 0, EVAL), "zxp_to_n_domain: operand 9 of kind 8"),
    "xdiv": (_opn(9, 0, XDIV), "zxp_to_n_domain: operand 9 of kind 9"),
    "xdivw": (_opn(9, 0, XDIVW), "zxp_to_n_domain: operand 9 of kind 10"),
    "kind_unknown": (_opn(7, 0, 13), "zxp_to_n_domain: operand 7 of kind 13"),
    "n_section": (_opn(2, 1, SEC_CM1_N), "zxp_to_n_domain: operand 2 names section 0"),
    "tmp_n_section": (_opn(6, 1, SEC_TMP_N), "zxp_to_n_domain: operand 6 names section 3"),
    "cm4_section": (_opn(6, 1, SEC_CM4_2NS), "zxp_to_n_domain: operand 6 names section 8"),
    "f_section": (_opn(5, 1, SEC_F_2NS), "zxp_to_n_domain: operand 5 names section 11"),
    "section_unknown": (_opn(6, 1, 12), "zxp_to_n_domain: operand 6 names section 12"),
    "instr_a_range": (_ins(2, 2, 13), "zxp_to_n_domain: instruction 2 out of range"),
    "instr_b_range": (_ins(0, 3, 13), "zxp_to_n_domain: instruction 0 out of range"),
    "instr_dst_range": (_ins(8, 1, 13), "zxp_to_n_domain: instruction 8 out of range"),
    "instr_op": (_ins(3, 0, 4), "zxp_to_n_domain: instruction 3 out of range"),
}


def test_base_program_is_accepted():
    import zkgpu
    ins, opn = base()
    got = zkgpu.zxp_to_n_domain(ins.astype(np.uint32), opn.astype(np.uint32), 1)
    assert np.array_equal(got, cc.to_n_domain(ins, opn, 1))
    # the negative multiple is accepted and becomes -1; 2 -> 1, 4 -> 2; ZI -> LIT 1; q as it is
    assert got[4].tolist() == [COL3, 1, 0, 0xFFFFFFFF]
    assert got[3].tolist() == [COL, 0, 1, 1] and got[5].tolist() == [COL3, 2, 0, 2]
    assert got[11].tolist() == [LIT, 1, 0, 0] and got[12].tolist() == [COL3, SEC_Q_2NS, 0, 0]
    # extend_bits 0: shifts stay
    o0 = opn.copy()
    o0[3, 3] = 1
    assert zkgpu.zxp_to_n_domain(ins.astype(np.uint32), o0.astype(np.uint32), 0)[3].tolist() == [COL, 0, 1, 1]


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refused(name):
    import zkgpu
    mutate, message = REFUSED[name]
    ins, opn = base()
    mutate(ins, opn)
    with pytest.raises(cc.Refused):
        cc.to_n_domain(ins.astype(np.uint32), opn.astype(np.uint32), 1)
    with pytest.raises(zkgpu.ZkgpuError) as e:
        zkgpu.zxp_to_n_domain(ins.astype(np.uint32), opn.astype(np.uint32), 1)
    assert str(e.value) == "zkgpu_zxp_to_n_domain failed (%d): %s" % (ERR_ARG, message)


def test_every_refusal_has_its_own_message():
    msgs = [m for _, m in REFUSED.values()]
    assert len(set(msgs)) == len(msgs)


# ---- semantics, on the oracle alone
ALPHA = [0x123456789ABCDEF, 7, P - 5]


@pytest.fixture(scope="module", params=[1, 2], ids=["blowup1", "blowup2"])
def inst(request):
    return instance((10, request.param, 100, 16))


def _proved(oracle, inst, rows=()):
    from oracle.stark_prover import OracleStark
    o = OracleStark(inst)
    o.witness()
    cc.corrupt(o, rows)
    o.prove()
    return o


def test_clean_trace_has_no_failing_row(oracle, inst):
    o = _proved(oracle, inst)
    assert cc.oracle_check(o, ALPHA) == (0, [], [0, 0, 0])


@pytest.mark.parametrize("rows", [(0,), (517,), (1023,), (3, 1023)], ids=lambda r: "-".join(map(str, r)))
def test_corrupted_trace_fails_at_exactly_those_rows(oracle, inst, rows):
    o = _proved(oracle, inst, rows)
    n_bad, bad, value = cc.oracle_check(o, ALPHA)
    assert (n_bad, bad) == (len(rows), sorted(rows))
    assert any(value)
