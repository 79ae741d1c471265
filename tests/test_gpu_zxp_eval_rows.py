"""zkgpu_zxp_eval_rows_dev (csrc/stark.hip k_zxp_eval_rows): an expression
program at a list of rows held in device memory, its stores compact.  Against
the CPU oracle's whole-domain evaluation read at the listed rows, for three
programs that exercise different operand kinds:
  tapped   the tapped n-domain step42ns, 2^10 rows: reads at row shift +1, wrapping at dom - 1
  quotient step42ns as is, 2^11 rows: X and ZI
  fri      step52ns, 2^11 rows, its f output compact: XDIV / XDIVW / EVAL
at list lengths around the wave's 64 lanes (130: three waves, the last
ragged), lists unsorted with repeats, rows 0 and dom - 1 and UINT64_MAX
entries, a whole wave of those, a list of nothing else.  The destination has
ld > n_rows, a sentinel everywhere and a guard word behind it: places that
are not listed, rows [n_rows, ld) and the guard keep the sentinel.  Every
refusal is ZKGPU_ERR_ARG with nothing written."""
import ctypes

import numpy as np
import pytest

import check_cases as cc
import split_cases as sc

pytestmark = pytest.mark.gpu

P = cc.P
MAX = 2**64 - 1
SENTINEL = 0xDEADBEEFCAFEF00D
ALPHA = [7, 1 << 33, P - 2]
SEC_Q, SEC_F = cc.SEC_Q_2NS, cc.SEC_F_2NS


@pytest.fixture(scope="module")
def world(zkgpu, oracle):
    """the oracle after a proof of the 2^10 instance, its sections on the device (column-major) and
    per program: (program, sections it reads, log_dom, challenges, evals, extras, output section,
    reference (dom, ncols) canonical)"""
    import bench
    from oracle import oracle as oc
    from oracle.stark_prover import OracleStark, _p
    inst = bench.stark_instance(10, 1, 100, 16, False)
    o = OracleStark(inst)
    o.witness()
    # (on a trace that satisfies the AIR every term is zero on every row: every third row and the
    # last break triple 0's and triple 1's identities, so that the taps have something to show)
    for r in list(range(0, o.N, 3)) + [o.N - 1]:
        for c in (2, 5):
            o.S[0][r, c] = (int(o.S[0][r, c]) + 1) % P
    o.prove()
    q_ref = o.S[SEC_Q].copy() % np.uint64(P)
    f_ref = o.S[SEC_F].copy() % np.uint64(P)
    terms, v = sc.oracle_terms(o, ALPHA)  # (overwrites S[SEC_Q])
    dev = {k: (zkgpu.to_device(np.ascontiguousarray(a.T)), a.shape[0], a.shape[1]) for k, a in o.S.items()
           if k not in (SEC_Q, SEC_F)}
    ch = np.array(o.challenges, np.uint64).reshape(8, 3)
    ch_a = ch.copy()
    ch_a[4] = np.array(ALPHA, np.uint64)
    xdiv = np.zeros((o.NE, 3), np.uint64)
    xdivw = np.zeros((o.NE, 3), np.uint64)
    oc.lib().oc_xdivxsub(_p(xdiv), _p(xdivw), _p(o.x_2ns), o.NE, _p(ch[7].copy()), oc.gl_w(inst.n_bits))
    extras = {"xdiv": zkgpu.to_device(xdiv.reshape(-1)), "xdivw": zkgpu.to_device(xdivw.reshape(-1)),
              "extend_bits": inst.blowup_bits, "x_start": 7}
    tapped = sc.TappedProgram(inst.programs["step42ns"], inst.blowup_bits)
    return {
        "o": o, "dev": dev,
        "tapped": (tapped, 10, ch_a, None, {}, SEC_Q, v.reshape(o.N, -1)),
        "quotient": (inst.programs["step42ns"], 11, ch, None, {"extend_bits": inst.blowup_bits, "x_start": 7}, SEC_Q,
                     q_ref),
        "fri": (inst.programs["step52ns"], 11, ch, o.evals, extras, SEC_F, f_ref),
    }


def _list(n, dom, seed):
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, dom, n, dtype=np.uint64)
    rows[0] = dom - 1
    if n >= 16:
        rows[1] = 0
        rows[5] = rows[2]          # a repeat
        rows[9] = rows[0]
        rows[7] = MAX
        rows[n - 2] = MAX
        rows[11] = dom             # the first index past the domain
    if n == 130:
        rows[64:128] = MAX         # a whole wave with nothing to do
    return rows


def _run(zkgpu, world, which, rows, n_rows=None, ld=None, rows_dev="upload"):
    prog, log_dom, ch, evals, extras, out_sec, ref = world[which]
    n_rows = len(rows) if n_rows is None else n_rows
    ncols = ref.shape[1]
    ld = n_rows + 5 if ld is None else ld
    dst = zkgpu.to_device(np.full(ncols * ld + 1, SENTINEL, np.uint64))
    secs = dict(world["dev"])
    secs[out_sec] = (dst, ld, ncols)
    drows = zkgpu.to_device(np.asarray(rows, np.uint64)) if rows_dev == "upload" else rows_dev
    try:
        zkgpu.zxp_eval_rows_dev(prog, secs, log_dom, ch, world["o"].publics, drows, n_rows, evals=evals, **extras)
    except zkgpu.ZkgpuError:  # a refusal queues nothing
        zkgpu.synchronize()
        assert np.array_equal(zkgpu.from_device(dst), np.full(ncols * ld + 1, SENTINEL, np.uint64))
        raise
    zkgpu.synchronize()
    return zkgpu.from_device(dst), ld, ncols, ref


def _expect(rows, n_rows, ld, ncols, ref, dom):
    want = np.full(ncols * ld + 1, SENTINEL, np.uint64)
    w = want[:-1].reshape(ncols, ld)
    for j in range(n_rows):
        if int(rows[j]) < dom:
            w[:, j] = ref[int(rows[j])]
    return want


@pytest.mark.parametrize("n", [1, 16, 63, 64, 65, 130])
@pytest.mark.parametrize("which", ["tapped", "quotient", "fri"])
def test_listed_rows_equal_the_oracle(zkgpu, world, which, n):
    dom = 1 << world[which][1]
    rows = _list(n, dom, 100 + n)
    got, ld, ncols, ref = _run(zkgpu, world, which, rows)
    assert ref.any() and ref.shape[0] == dom
    assert np.array_equal(got, _expect(rows, n, ld, ncols, ref, dom))


@pytest.mark.parametrize("which", ["tapped", "fri"])
def test_a_list_of_nothing(zkgpu, world, which):
    dom = 1 << world[which][1]
    for rows in (np.full(16, MAX, np.uint64), np.array([dom, MAX, dom + 5] * 30, np.uint64)):
        got, ld, ncols, ref = _run(zkgpu, world, which, rows)
        assert np.array_equal(got, np.full(ncols * ld + 1, SENTINEL, np.uint64))


def test_only_the_first_n_rows_of_the_list_count(zkgpu, world):
    rows = _list(65, 1 << 10, 3)
    got, ld, ncols, ref = _run(zkgpu, world, "tapped", rows, n_rows=20, ld=32)
    assert np.array_equal(got, _expect(rows, 20, 32, ncols, ref, 1 << 10))
    got, ld, ncols, ref = _run(zkgpu, world, "tapped", rows, n_rows=0, ld=4)
    assert np.array_equal(got, np.full(ncols * 4 + 1, SENTINEL, np.uint64))


def test_refusals(zkgpu, world):
    from zkgpu import ZkgpuError
    rows = _list(16, 1 << 10, 5)

    def refused(message, which="tapped", **kw):
        with pytest.raises(ZkgpuError) as e:
            _run(zkgpu, world, which, rows, **kw)
        assert str(e.value) == "zkgpu_zxp_eval_rows_dev failed (-2): " + message

    refused("zxp rows: section %d is stored to and holds 15 rows, not 16" % SEC_Q, ld=15)
    refused("zxp rows: 4097 rows exceed 4096", n_rows=4097, ld=4100)
    refused("zxp rows: null row list", rows_dev=None)
    # a section both read and stored to; a store at a row shift (small programs over cm1_n / q)
    o = world["o"]
    one = np.zeros(24, np.uint64)
    drows = zkgpu.to_device(rows)
    for ins, opn, secs_extra, message in [
        ([(cc.COPY, 0, 1, 0)], [(cc.COL, cc.SEC_CM1_N, 0, 0), (cc.COL, cc.SEC_CM1_N, 1, 0)], {},
         "zxp rows: section 0 is both read and stored to"),
        ([(cc.COPY, 0, 1, 0)], [(cc.COL, SEC_Q, 0, 1), (cc.COL, cc.SEC_CM1_N, 1, 0)], {SEC_Q: 1},
         "zxp rows: instruction 0 stores at row shift 1"),
    ]:
        cm1 = zkgpu.to_device(np.ascontiguousarray(o.S[0].T))
        secs = {cc.SEC_CM1_N: (cm1, o.N, o.S[0].shape[1])}
        dst = zkgpu.to_device(np.full(64, SENTINEL, np.uint64))
        for s, nc in secs_extra.items():
            secs[s] = (dst, 32, nc)
        with pytest.raises(ZkgpuError) as e:
            zkgpu.zxp_eval_rows_dev((np.array(ins, np.uint32), np.array(opn, np.uint32), 1, 1), secs, 10, one, None,
                                    drows, 16)
        assert str(e.value) == "zkgpu_zxp_eval_rows_dev failed (-2): " + message
        zkgpu.synchronize()
        assert np.array_equal(zkgpu.from_device(cm1).astype(np.uint64).reshape(-1, o.N).T, o.S[0])
        assert np.array_equal(zkgpu.from_device(dst).astype(np.uint64), np.full(64, SENTINEL, np.uint64))
