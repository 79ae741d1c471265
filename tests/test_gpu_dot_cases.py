"""The dot-product layer on the GPU at worst-case operands (tests/dot_cases.py).

Expression programs: every builder, on worst-case and on random inputs,
through zkgpu.zxp_eval_dev as a run-time compiled kernel, on the interpreter
at three term caps and as the unfused source; every section equals the
oracle's evaluation of the SOURCE program bit for bit.  Evaluation map:
zkgpu.evmap_dev with pool coefficients in LEv / LpEv and A_MAX columns
against Python-integer sums and oc_evmap.

Lazy columns: zkgpu_load_rows_dev and k_rows_to_cols (csrc/ntt.hip) copy host
words unchanged and zkgpu_stark_set_cm1 goes through them, so a non-canonical
word (p .. 2^64 - 1) of a caller's trace reaches a section as it is; the
compiled programs must take it.  test_lazy_columns feeds wide_sum(250) with
columns at 2^64 - 1 in every mode, against Python integers and against the
oracle on the same input reduced mod p.
"""
import ctypes

import numpy as np
import pytest

import dot_cases as dc

pytestmark = pytest.mark.gpu

P = dc.P
COMPILED = [("1", "0", "2"), ("1", "256", "2")]
INTERP = [("1", "0", "0"), ("1", "256", "0"), ("1", "3", "0"), ("0", "0", "0")]

BUILDERS = {
    "wide_sum_249": lambda: dc.wide_sum(249), "wide_sum_250": lambda: dc.wide_sum(250),
    "wide_sum_251": lambda: dc.wide_sum(251), "wide_sum_500": lambda: dc.wide_sum(500),
    "wide_sum_700": lambda: dc.wide_sum(700), "wide_sum_250_dim1": lambda: dc.wide_sum(250, 1),
    "chains_800": lambda: dc.chains(800), "combine_store_200": lambda: dc.combine_store(200, 200),
    "combine_store_256": lambda: dc.combine_store(256, 256), "temp_terms_90": lambda: dc.temp_terms(90),
}
JIT_NAMES = ["wide_sum_250", "wide_sum_500", "wide_sum_250_dim1", "chains_800", "combine_store_256", "temp_terms_90"]
_memo = {}


def _reference(oracle, name, worst):
    """(case, inputs, the oracle's sections after the source program), once
    per (builder, input kind); never written to afterwards."""
    key = (name, worst)
    if key not in _memo:
        if name not in _memo:
            _memo[name] = BUILDERS[name]()
        c = _memo[name]
        inp = dc.Inputs(c, worst == "worst", seed=sum(map(ord, name)), chal_one=worst == "worst")
        _memo[key] = (c, inp, dc.oracle_eval(oracle, c, inp))
    return _memo[key]


def _run_gpu(zkgpu, c, inp, S):
    import torch
    secs = {k: (zkgpu.to_device(np.ascontiguousarray(a.T)), inp.dom, a.shape[1]) for k, a in S.items()}
    zkgpu.zxp_eval_dev(c.prog, secs, dc.LOG_DOM, inp.chal, inp.pub, inp.evals)
    torch.cuda.synchronize()
    return {k: zkgpu.from_device(t).T for k, (t, _, _) in secs.items()}


def _set_mode(monkeypatch, mode):
    monkeypatch.setenv("ZKGPU_ZXP_FUSE", mode[0])
    monkeypatch.setenv("ZKGPU_ZXP_MAX_TERMS", mode[1])
    monkeypatch.setenv("ZKGPU_ZXP_JIT", mode[2])


def _cases():
    out = [(n, m) for n in JIT_NAMES for m in COMPILED]
    out += [(n, m) for n in sorted(BUILDERS) for m in INTERP]
    # chains with random challenges is the ordinary Horner case: "horner"
    return [pytest.param(n, m, w, id="%s-%s-%s" % (n, "".join(m), w)) for n, m in out
            for w in (("worst", "random", "horner") if n.startswith("chains") else ("worst", "random"))]


@pytest.mark.parametrize("name,mode,worst", _cases())
def test_programs_vs_oracle(oracle, zkgpu, monkeypatch, name, mode, worst):
    _set_mode(monkeypatch, mode)
    if worst == "horner":  # worst-case columns and evals under random challenges
        key = (name, "horner")
        if key not in _memo:
            c = _reference(oracle, name, "worst")[0]
            inp = dc.Inputs(c, True, seed=77, chal_one=False)
            _memo[key] = (c, inp, dc.oracle_eval(oracle, c, inp))
        c, inp, want = _memo[key]
    else:
        c, inp, want = _reference(oracle, name, worst)
    got = _run_gpu(zkgpu, c, inp, inp.S)
    for k in c.widths:
        bad = np.argwhere(got[k] != want[k])
        assert bad.size == 0, "section %d: %d cells differ, first at row %d col %d" % (k, len(bad), *bad[0])


@pytest.mark.parametrize("mode", COMPILED + INTERP, ids=lambda m: "".join(m))
def test_lazy_columns(oracle, zkgpu, monkeypatch, mode):
    """wide_sum(250) with every column word at 2^64 - 1 (rows 0..255) and
    random u64 of which half are >= p (the rest): the stored sums equal the
    Python-integer sums of the words as they are, and the oracle's run on
    the same columns reduced mod p."""
    _set_mode(monkeypatch, mode)
    key = ("lazy",)
    if key not in _memo:
        c = dc.wide_sum(250)
        inp = dc.Inputs(c, True, seed=31)
        rng = np.random.default_rng(32)
        lazy = rng.integers(0, 1 << 64, size=inp.S[dc.SEC_IN].shape, dtype=np.uint64, endpoint=False)
        lazy[:, ::2] |= np.uint64(0xFFFFFFFF00000001)  # >= p
        lazy[:256] = dc.M64
        S_or = inp.sections()
        S_or[dc.SEC_IN] = lazy % np.uint64(P)
        want = dc.oracle_eval(oracle, c, inp, S=S_or)
        rows = [0, 100, 255, 256, 700, inp.dom - 1]
        _memo[key] = (c, inp, lazy, want, rows, dc.wide_sum_rows(250, 3, inp, rows, cols=lazy))
    c, inp, lazy, want, rows, ref = _memo[key]
    S = inp.sections()
    S[dc.SEC_IN] = lazy
    got = _run_gpu(zkgpu, c, inp, S)
    assert np.array_equal(got[dc.SEC_IN], lazy)  # read-only: left as loaded
    for i, r in zip(rows, ref):
        assert [int(x) for x in got[dc.SEC_OUT][i]] == r, "row %d" % i
    assert np.array_equal(got[dc.SEC_OUT], want[dc.SEC_OUT])


# ---------------------------------------------------------------- evaluation map
EV_ENTRIES = [(0, 1, 0), (1, 1, 1), (2, 3, 0), (2, 3, 1), (6, 1, 0), (5, 3, 1), (8, 1, 1), (7, 1, 0), (3, 3, 0)]
EV_ROWS = 61440  # rows per block of k_evmap_groups: 256 threads x 240 rows (csrc/stark.hip)


def _evmap_reference(cols, lev, lpev, n, eb):
    """sum_k L(k) p_j[k] mod p per sub-entry as exact integers, recombined
    with x^3 = x + 1.  Both factors are cut into 16-bit pieces: a piece
    product is below 2^32 and n < 2^17 of them sum below 2^49, exact in
    uint64 (n 2^32 < 2^64 in general); the 16 piece sums of a pair are put
    together in Python integers."""
    def pieces(a):  # (rows, w) -> (w * 4, rows)
        return np.stack([(a.T >> np.uint64(16 * q)) & np.uint64(0xFFFF) for q in range(4)], axis=1).reshape(-1, len(a))

    assert n < 1 << 31
    C = pieces(cols[::1 << eb]).T  # (rows, 9 * 4)
    sums = {}
    for prime, L in ((0, lev), (1, lpev)):
        M = (pieces(L) @ C).reshape(3, 4, 9, 4)
        for t in range(3):
            for c in range(9):
                sums[prime, t, c] = sum(int(M[t, a, c, b]) << (16 * (a + b)) for a in range(4) for b in range(4))
    out = np.zeros((len(EV_ENTRIES), 3), np.uint64)
    for e, (c0, dim, prime) in enumerate(EV_ENTRIES):
        acc = [0, 0, 0]
        for j in range(dim):
            # S_j in F_p^3: component t = sum_k L_t(k) p_j[k]
            s = [sums[prime, t, c0 + j] for t in range(3)]
            # times X^j (X^3 = X + 1): (a0, a1, a2) X = (a2, a0 + a2, a1)
            for _ in range(j):
                s = [s[2], s[0] + s[2], s[1]]
            acc = [a + b for a, b in zip(acc, s)]
        out[e] = [a % P for a in acc]
    return out


def _evmap_cases():
    out = [(n, eb, kind) for n, eb in ((EV_ROWS + 300, 0), (2 * EV_ROWS, 1))
           for kind in ("worst", "worst_random_rows", "zero_lev")]
    # A thread takes n / 256 rows at most, whatever the block size: only
    # n >= 256 x 2^64 / (0.89 TERM_MAX) = 256 x 576 rows can show a rows-per-thread
    # count that is too high (0.89: the pool's mean share in A0).  640 rows
    # per thread and a ragged tail.
    return out + [(640 * 256 + 77, 0, "worst")]


@pytest.mark.parametrize("n,eb,kind", _evmap_cases())
def test_evmap_worst_case(oracle, zkgpu, n, eb, kind):
    """One full block of 240 rows per thread plus a ragged tail, two full
    blocks on an extended domain, and enough rows that a thread asked for 576
    or more of them would wrap; LEv / LpEv hold pool coefficients in all three
    components and every column word is A_MAX, so each thread's nine
    accumulators per sub-entry carry 240 near-maximal terms."""
    rng = np.random.default_rng(n + eb)
    ne = n << eb
    cols = np.full((ne, 9), dc.A_MAX, np.uint64)
    lev = dc.pool_values(rng, (n, 3))
    lpev = dc.pool_values(rng, (n, 3))
    if kind == "worst_random_rows":  # one random row in 64
        pick = np.arange(int(rng.integers(0, 64)), n, 64)
        lev[pick] = dc.rand_canon(rng, (len(pick), 3))
        lpev[pick] = dc.rand_canon(rng, (len(pick), 3))
        cols[pick << eb] = dc.rand_canon(rng, (len(pick), 9))
    if kind == "zero_lev":
        lev[:] = 0
    want = _evmap_reference(cols, lev, lpev, n, eb)
    ptrs = (ctypes.c_void_p * len(EV_ENTRIES))(*[cols.ctypes.data + 8 * c for c, _, _ in EV_ENTRIES])
    strides = np.full(len(EV_ENTRIES), 9, np.uint64)
    dims = np.array([d for _, d, _ in EV_ENTRIES], np.uint32)
    primes = np.array([p for _, _, p in EV_ENTRIES], np.uint32)
    ref = np.zeros((len(EV_ENTRIES), 3), np.uint64)
    oracle.lib().oc_evmap(oracle._p(ref), ctypes.cast(ptrs, ctypes.c_void_p), ctypes.c_void_p(strides.ctypes.data),
                          ctypes.c_void_p(dims.ctypes.data), ctypes.c_void_p(primes.ctypes.data), len(EV_ENTRIES),
                          oracle._p(lev), oracle._p(lpev), n, eb)
    assert np.array_equal(ref, want)  # the two references agree
    if kind == "zero_lev":
        assert not want[[e for e, (_, _, p) in enumerate(EV_ENTRIES) if not p]].any()
    dcols = zkgpu.to_device(np.ascontiguousarray(cols.T))
    dlev = zkgpu.to_device(np.ascontiguousarray(lev.T))
    dlpev = zkgpu.to_device(np.ascontiguousarray(lpev.T))
    base = dcols.data_ptr()
    got = zkgpu.evmap_dev([base + 8 * ne * c for c, _, _ in EV_ENTRIES], [ne] * len(EV_ENTRIES), dims, primes, dlev,
                          dlpev, n, n, eb)
    assert np.array_equal(got, want)


# ---------------------------------------------------------------- shapes left to the interpreter
def _shape_reference(oracle, name):
    """(case, inputs, the oracle's sections after the program), once per shape"""
    import jit_shape_cases as js
    key = ("shape", name)
    if key not in _memo:
        c = dc.Case(name, js.UNSUPPORTED[name](), 0, 0, 0)
        c.widths = dict(js.WIDTHS)
        inp = dc.Inputs(c, False, seed=sum(map(ord, name)))
        if name == "cross_row_read_after_write":
            # Row i reads cm2[0] of row i + 1 while that row stores it (rows run
            # in parallel, in the oracle too): the column already holds the
            # product the program stores, so the read has one value whichever
            # comes first -- as the stage-3 programs' shifted cells do.  Only
            # cm3 observes this program then: a lost store to cm2[0] would not show
            a = inp.S[js.SEC_CM1_N]
            inp.S[js.SEC_CM2_N][:, 0] = [int(x) * int(y) % P for x, y in zip(a[:, 0], a[:, 1])]
        _memo[key] = (c, inp, dc.oracle_eval(oracle, c, inp))
    return _memo[key]


@pytest.mark.parametrize("name", ["cross_row_read_after_write", "mixed_stored_triple"])
def test_unsupported_shapes_fall_back_to_the_interpreter(oracle, zkgpu, monkeypatch, name):
    """The two program shapes the source generator does not print
    (tests/jit_shape_cases.py; zxp_jit_source fails on them, test_zxp_compile)
    at 2^10 rows, where the shifted read wraps at the last row, with the
    compiled kernels forced (ZKGPU_ZXP_JIT=2): zxp_jit_run answers 1 and the
    interpreter runs them -- every section equals the oracle's evaluation and
    the run with ZKGPU_ZXP_JIT=0 bit for bit.  No hiprtc runs."""
    import jit_shape_cases as js
    c, inp, want = _shape_reference(oracle, name)
    with pytest.raises(RuntimeError, match="unsupported program shape"):
        zkgpu.zxp_jit_source(c.prog, inp.chal, inp.pub, inp.evals)
    assert not np.array_equal(want[js.SEC_CM3_N], inp.S[js.SEC_CM3_N])  # the program wrote
    got = {}
    for jit in ("2", "0"):
        _set_mode(monkeypatch, ("1", "0", jit))
        zkgpu.prof_reset()
        zkgpu.prof_enable(True)
        got[jit] = _run_gpu(zkgpu, c, inp, inp.S)
        zkgpu.prof_enable(False)
        ran = zkgpu.prof_kernels()
        assert "k_zxp_eval" in ran and not [k for k in ran if k.startswith("k_zxp_jit")], (jit, ran)
        for k in c.widths:
            bad = np.argwhere(got[jit][k] != want[k])
            assert bad.size == 0, "JIT=%s section %d: %d cells differ, first at row %d col %d" % (jit, k, len(bad), *bad[0])
    assert all(np.array_equal(got["2"][k], got["0"][k]) for k in c.widths)
