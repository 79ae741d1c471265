"""zkgpu_zxp_split_constraints (csrc/zxp_split.cpp): the constraint combination
of a quotient program taken apart into its terms.  The library against the
Python restatement of the rule (tests/split_cases.py) on the instances' own
step42ns, as given and after the n-domain rewrite; the identity the feature
rests on -- C = sum of (+/-) alpha^e v_k over the live terms -- on every row
of a 2^10 domain on the CPU oracle, clean and corrupted; one defective copy of
a small program per refusal.  CPU only.

The zkEVM-shaped instance: its generator lets an opcode whose F_p^3 operand
has no open value read slot 0, the accumulator (instruction 8:
TMP3[2] = TMP3[0] * CHAL[2], right after acc = 0 + CHAL[4]).  Nothing ever comes
of that product, so it spoils its slot and is dropped (the rule's last case);
the instance splits into 4621 terms, none dead."""
import numpy as np
import pytest

import check_cases as cc
import split_cases as sc
from check_cases import (ADD, CHAL, COL, COL3, COPY, LIT, MUL, SEC_CM1_2NS, SEC_CM2_2NS, SEC_Q_2NS, SUB, TMP1, TMP3,
                         ZI)

ERR_ARG = -2
M2 = 0xFFFFFFFE


def _inst(blow=1, kind=False):
    import bench
    return bench.stark_instance(10, blow, 100, 16, kind)


def _library(ins, opn, chal=4):
    import zkgpu
    try:
        return tuple(x.tolist() for x in zkgpu.zxp_split_constraints(ins, opn, chal))
    except zkgpu.ZkgpuError as e:
        return str(e)


def _restated(ins, opn, chal=4):
    try:
        return tuple(x.tolist() for x in sc.split(ins, opn, chal))
    except cc.Refused as e:
        return "zkgpu_zxp_split_constraints failed (%d): zxp_split: %s" % (ERR_ARG, e)


@pytest.mark.parametrize("n_domain", [False, True])
@pytest.mark.parametrize("which", ["blow1", "blow2", "zkevm"])
def test_library_equals_restatement(which, n_domain):
    inst = {"blow1": lambda: _inst(1), "blow2": lambda: _inst(2), "zkevm": lambda: _inst(1, "zkevm")}[which]()
    ins, opn = inst.programs["step42ns"].arrays()
    if n_domain:
        opn = cc.to_n_domain(ins, opn, inst.blowup_bits)
    got, want = _library(ins, opn), _restated(ins, opn)
    assert got == want
    assert not isinstance(want, str), want
    if which == "zkevm":  # acc = 0 + alpha, then (acc + c) * alpha: the literal 1, the 0, then the identities
        tapped, operands, terms = want
        k = len(terms)
        assert k > 1000 and terms[0] == [k - 1, 0, 0, 0] and terms[1] == [k - 2, 0, 0, 0] and terms[-1][0] == 1
        assert not any(t[1] or t[3] for t in terms) and len(tapped) <= 2 * ins.shape[0]
        assert ins[8].tolist() not in tapped  # the spoiled product is gone
        return
    tapped, operands, terms = want
    k = len(terms)
    assert k > 16 and len(tapped) <= 2 * ins.shape[0] and len(operands) <= opn.shape[0] + 2 * ins.shape[0] + 1
    # the synthetic form acc = acc * alpha + C_k: term t at exponent k - t, none negated or dead
    assert [t[0] for t in terms] == list(range(k - 1, -1, -1)) and not any(t[1] or t[3] for t in terms)
    assert [t[2] for t in terms] == sorted(t[2] for t in terms)
    # no instruction of the tapped program reads the challenge or stores outside its own columns
    for op, d, a, b in tapped:
        assert not any(operands[s][:2] == [CHAL, 4] for s in ([a] if op == COPY else [a, b]))
        if operands[d][0] in (COL, COL3):
            assert operands[d][0] == COL3 and operands[d][1] == SEC_Q_2NS and operands[d][2] % 3 == 0


@pytest.mark.parametrize("rows", [(), (0,), (517,), (3, 1023)])
def test_terms_sum_to_the_combination_on_every_row(oracle, rows):
    from oracle.stark_prover import OracleStark
    o = OracleStark(_inst())
    o.witness()
    cc.corrupt(o, rows)
    o.prove()
    alpha = [5, 1 << 40, cc.P - 3]
    n_bad, bad, _ = cc.oracle_check(o, alpha)
    c = (o.S[SEC_Q_2NS] % np.uint64(cc.P)).copy()
    assert (n_bad, bad) == (len(rows), sorted(rows))
    # the tapped program and the terms are the LIBRARY's (and equal the restatement's)
    import zkgpu
    terms, v = sc.oracle_terms(o, alpha, split=zkgpu.zxp_split_constraints)
    terms_r, v_r = sc.oracle_terms(o, alpha)
    assert np.array_equal(terms, terms_r) and np.array_equal(v, v_r)
    live = [t for t in range(terms.shape[0]) if not terms[t, 3]]
    for r in range(o.N):
        assert sc.combine(terms, v[r, live], alpha) == [int(x) for x in c[r]], r
    for r in range(o.N):
        ids, _ = sc.named(terms, v, r)
        assert ids == ([0] if r in rows else []), r


# ---------------------------------------------------------------- a small program and its defects
def base():
    opn = [(TMP1, 0, 0, 0), (TMP3, 0, 0, 0), (COL, SEC_CM1_2NS, 0, 0), (COL, SEC_CM1_2NS, 1, 2),
           (COL3, SEC_CM2_2NS, 0, M2), (CHAL, 4, 0, 0), (LIT, 5, 0, 0), (ZI, 0, 0, 0), (COL3, SEC_Q_2NS, 0, 0),
           (TMP3, 1, 0, 0), (CHAL, 2, 0, 0), (COL3, SEC_Q_2NS, 3, 0), (COL, SEC_CM1_2NS, 2, 0)]
    ins = [(MUL, 0, 2, 3), (MUL, 1, 0, 5), (SUB, 0, 2, 6), (ADD, 1, 1, 0), (MUL, 1, 5, 1), (SUB, 9, 4, 1),
           (MUL, 8, 9, 7)]
    return ins, opn


def test_small_program():
    ins, opn = base()
    want = _restated(ins, opn)
    assert _library(ins, opn) == want
    tapped, operands, terms = want
    k = len(opn)
    assert operands == [list(o) for o in opn] + [[COL3, SEC_Q_2NS, 0, 0], [COL3, SEC_Q_2NS, 3, 0],
                                                 [COL3, SEC_Q_2NS, 6, 0]]
    assert tapped == [[MUL, 0, 2, 3], [COPY, k, 0, 0], [SUB, 0, 2, 6], [COPY, k + 1, 0, 0], [COPY, k + 2, 4, 0]]
    # q = c4 - ((t0 * alpha + t1) * alpha)
    assert terms == [[2, 1, 1, 0], [1, 1, 3, 0], [0, 0, 5, 0]]


def test_reads_of_the_challenge_and_dead_terms():
    """acc = 0 + alpha (a never-zero term 0 = the literal 1, then the 0), (acc + c) * alpha, a COPY
    to q; a combination left in a slot is dead"""
    opn = [(TMP3, 0, 0, 0), (LIT, 0, 0, 0), (CHAL, 4, 0, 0), (COL, SEC_CM1_2NS, 0, 0), (TMP3, 1, 0, 0),
           (COL3, SEC_Q_2NS, 0, 0), (TMP3, 2, 0, 0)]
    ins = [(ADD, 0, 1, 2), (ADD, 4, 0, 3), (MUL, 0, 4, 2), (MUL, 6, 3, 2), (COPY, 5, 0, 0)]
    want = _restated(ins, opn)
    assert _library(ins, opn) == want
    tapped, operands, terms = want
    assert operands[len(opn):] == [[LIT, 1, 0, 0], [COL3, SEC_Q_2NS, 0, 0], [COL3, SEC_Q_2NS, 3, 0],
                                   [COL3, SEC_Q_2NS, 6, 0], [COL3, SEC_Q_2NS, 9, 0]]
    assert tapped == [[COPY, 8, 7, 0], [COPY, 9, 1, 0], [COPY, 10, 3, 0], [COPY, 11, 3, 0]]
    assert terms == [[2, 0, 0, 0], [1, 0, 0, 0], [1, 0, 1, 0], [0, 0, 3, 1]]


def test_a_product_that_feeds_nothing_is_dropped():
    """TMP3[2] = acc * CHAL[2] and what is computed from it alone, never read by the combination"""
    ins, opn = base()
    k = len(opn)
    opn += [(TMP3, 2, 0, 0), (TMP3, 3, 0, 0)]
    plain = _restated(ins, opn)
    ins[4:4] = [(MUL, k, 1, 10), (ADD, k + 1, k, 2), (COPY, k, k + 1, 0)]
    want = _restated(ins, opn)
    assert _library(ins, opn) == want
    assert want[0] == plain[0] and want[1] == plain[1]
    assert [t[:2] + t[3:] for t in want[2]] == [t[:2] + t[3:] for t in plain[2]]
    assert [t[2] for t in want[2]] == [1, 3, 8]
    # ... until it would count: added to the combination, multiplied by the challenge, stored
    for extra, at in [((ADD, 1, 1, k), 7), ((MUL, k, k, 5), 7), ((COPY, 12, k, 0), 7), ((SUB, 0, k, 2), 7)]:
        bad = list(ins)
        bad.insert(at, extra)
        msg = ("zkgpu_zxp_split_constraints failed (%d): zxp_split: instruction 4 multiplies a combination by "
               "something other than the combination challenge" % ERR_ARG)
        assert _restated(bad, opn) == msg and _library(bad, opn) == msg
    # overwritten by a plain value the slot is plain again
    ok = list(ins)
    ok[7:7] = [(COPY, k, 2, 0), (ADD, 1, 1, k)]
    got = _restated(ok, opn)
    assert _library(ok, opn) == got and len(got[2]) == 4


DEFECTS = [
    ("product_by_another_challenge", 4, (MUL, 1, 1, 10),
     "instruction 4 multiplies a combination by something other than the combination challenge"),
    ("product_of_two_combinations", 5, (MUL, 9, 1, 1),
     "instruction 5 multiplies a combination by something other than the combination challenge"),
    ("zi_into_a_temporary", 6, (MUL, 9, 9, 7), "no combination is stored to SEC_Q_2NS"),
    ("product_into_tmp1", 4, (MUL, 0, 1, 10),
     "instruction 4 multiplies a combination by something other than the combination challenge"),
    ("tmp1_destination", 3, (ADD, 0, 1, 0), "instruction 3 writes a combination to a TMP1 slot"),
    ("q_column_3", 6, (MUL, 11, 9, 7),
     "instruction 6 stores a combination to a column other than q (SEC_Q_2NS, column 0, shift 0)"),
    ("cm1_column", 6, (COPY, 12, 9, 0),
     "instruction 6 stores a combination to a column other than q (SEC_Q_2NS, column 0, shift 0)"),
    ("read_only_destination", 6, (COPY, 6, 9, 0), "instruction 6 writes a combination to an operand of kind 4"),
    ("q_by_a_sum", 6, (ADD, 8, 9, 0),
     "instruction 6 stores a combination to q other than by a COPY or a product by ZI or 1"),
    ("q_by_a_product_by_the_challenge", 6, (MUL, 8, 9, 5),
     "instruction 6 stores a combination to q other than by a COPY or a product by ZI or 1"),
    ("alpha_free_store_to_q", 6, (COPY, 8, 0, 0),
     "instruction 6 stores a value free of the combination challenge to SEC_Q_2NS"),
    ("second_store_to_q", 7, (COPY, 8, 9, 0), "instruction 7 is a second store to q"),
    ("shared_term", 5, (ADD, 9, 1, 1), "instruction 5 combines two combinations that share term 0"),
    ("no_store", 6, None, "no combination is stored to SEC_Q_2NS"),
    ("source_out_of_range", 2, (SUB, 0, 13, 6), "instruction 2 out of range"),
    ("second_source_out_of_range", 0, (MUL, 0, 2, 13), "instruction 0 out of range"),
    ("destination_out_of_range", 6, (MUL, 13, 9, 7), "instruction 6 out of range"),
    ("unknown_op", 3, (4, 1, 1, 0), "instruction 3 out of range"),
]


@pytest.mark.parametrize("name,k,instr,message", DEFECTS, ids=[d[0] for d in DEFECTS])
def test_refusals(name, k, instr, message):
    ins, opn = base()
    if instr is None:
        del ins[k]
    elif k == len(ins):
        ins.append(instr)
    else:
        ins[k] = instr
    want = "zkgpu_zxp_split_constraints failed (%d): zxp_split: %s" % (ERR_ARG, message)
    assert _restated(ins, opn) == want
    assert _library(ins, opn) == want


def test_challenge_out_of_range():
    ins, opn = base()
    assert _library(ins, opn, 8) == _restated(ins, opn, 8) == (
        "zkgpu_zxp_split_constraints failed (%d): zxp_split: challenge 8 out of range" % ERR_ARG)
