"""zkgpu_zxp_eval_block_dev, the expression evaluator over one row block of a
row-sharded domain (host/sharded_starks.hpp run_n / run_block), against the
oracle's evaluation of the WHOLE domain, bit for bit (tests/block_cases.py is
the model, tests/test_block_cases.py checks it on the CPU).

Every block of a domain is loaded as the local image its owner holds -- its
rows, the halo rows of the next block, pad rows and guard words of a poison
value -- and evaluated by one call with x_start = (7) w^row0 and the xdiv
arrays advanced to row0.  Afterwards the whole image must be what the model
says: the stored regions (a store at shift s on local rows [s, 2^log_rows +
s)) hold the oracle's whole-domain values, every other word is as loaded;
and all blocks' stored regions recompose to the oracle's sections.

a. three hand-built programs x block sizes (the whole domain as one block, a
   quarter, one interpreter workgroup, fewer rows than a wave) x ld at its
   bound or 3 rows above x the run-time compiled kernel, the interpreter at
   two term caps and the unfused source; inputs half non-canonical words
b. the zkEVM-shaped step3 / step42ns / step52ns programs whose compiled
   kernels build() caches, on 4 blocks (compiled, segments with scratch
   columns of a block's ld) and 2 blocks (interpreter) of a 2^12 domain
c. what the call refuses, with nothing queued
"""
import numpy as np
import pytest

import block_cases as bc

pytestmark = pytest.mark.gpu

P = bc.P
MODES = [("1", "0", "2"), ("1", "0", "0"), ("1", "3", "0"), ("0", "0", "0")]  # (FUSE, MAX_TERMS, JIT)
_memo = {}


def _set_mode(monkeypatch, mode):
    monkeypatch.setenv("ZKGPU_ZXP_FUSE", mode[0])
    monkeypatch.setenv("ZKGPU_ZXP_MAX_TERMS", mode[1])
    monkeypatch.setenv("ZKGPU_ZXP_JIT", mode[2])


def _run_blocks(zkgpu, prog, loaded, widths, g, ext, eb, chal, pub, evals, xdiv=None, xdivw=None):
    """One zxp_eval_block_dev call per block on its uploaded image -> the
    images afterwards, per block.  (The blocks' images of a section sit back
    to back in one device buffer: each call sees only its own.)"""
    import torch
    dev = {sec: zkgpu.to_device(np.stack([blk[sec] for blk in loaded])) for sec in widths}
    dx = [zkgpu.to_device(a.reshape(-1)) if a is not None else None for a in (xdiv, xdivw)]
    for b in range(g.nblocks):
        row0 = g.row0(b)
        secs = {sec: (dev[sec].data_ptr() + 8 * b * g.words(w), g.ld, w) for sec, w in widths.items()}
        # xdiv / xdivw: the whole arrays from word 3 row0 on
        xd = [t.data_ptr() + 8 * 3 * row0 if t is not None else None for t in dx]
        zkgpu.zxp_eval_block_dev(prog, secs, g.log_rows, g.log_domain, chal, pub, evals, xdiv=xd[0], xdivw=xd[1],
                                 extend_bits=eb, x_start=bc.x_start(g.log_domain, row0, ext))
    torch.cuda.synchronize()
    host = {sec: zkgpu.from_device(t) for sec, t in dev.items()}
    return [{sec: host[sec][b] for sec in widths} for b in range(g.nblocks)]


def _check_blocks(got, S_loaded, S_after, stores, widths, g):
    want = bc.expected(S_loaded, S_after, stores, g)
    for b in range(g.nblocks):
        bc.assert_block(got[b], want[b], widths, g, b)
    bc.assert_recomposed(got, stores, S_after, widths, g)


# ---------------------------------------------------------------- a. hand-built programs
def _reference(oracle, name):
    """(case, inputs, the oracle's whole-domain sections), once per case; never written to"""
    if name not in _memo:
        case = bc.CASES[name]()
        inp = bc.Inputs(case, seed=sum(map(ord, name)))
        _memo[name] = (case, inp, bc.oracle_whole(oracle, case, inp))
    return _memo[name]


def _cases():
    return [pytest.param(n, lr, pad, m, id="%s-r%d-pad%d-%s" % (n, lr, pad, "".join(m)))
            for n in bc.CASES for m in MODES for lr in bc.LOG_ROWS[n] for pad in bc.PADS]


@pytest.mark.parametrize("name,log_rows,pad,mode", _cases())
def test_blocks_equal_the_whole_domain(oracle, zkgpu, monkeypatch, name, log_rows, pad, mode):
    _set_mode(monkeypatch, mode)
    case, inp, after = _reference(oracle, name)
    g = bc.Geom(case.log_domain, log_rows, case.halo, pad)
    loaded = bc.split(inp.S, g.log_domain, g.log_rows, g.halo, g.pad, g.guard)
    zkgpu.prof_reset()
    zkgpu.prof_enable(True)
    try:
        got = _run_blocks(zkgpu, case.prog, loaded, case.widths, g, case.ext, case.eb, inp.chal, inp.pub, inp.evals,
                          inp.xdiv if case.ext else None, inp.xdivw if case.ext else None)
    finally:
        zkgpu.prof_enable(False)
    ran = zkgpu.prof_kernels()
    if mode[2] == "2":
        assert "k_zxp_jit" in ran and "k_zxp_eval" not in ran, ran
    else:
        assert "k_zxp_eval" in ran and not [k for k in ran if k.startswith("k_zxp_jit")], ran
    _check_blocks(got, inp.S, after, case.stores, case.widths, g)


# ---------------------------------------------------------------- b. zkEVM-shaped programs
SEC_CONST_N, SEC_CONST_2NS, SEC_Q_2NS, SEC_F_2NS = 4, 9, 10, 11
LOG_DOM = 12


def _rand(rng, shape):
    return rng.integers(0, P, size=shape, dtype=np.uint64)


def _shaped_reference(oracle, zkgpu, name):
    """(program, stores, halo, widths, sections before, after the oracle's
    whole-domain oc_parser_eval, scalars, xdiv, xdivw), once per program"""
    key = ("shaped", name)
    if key in _memo:
        return _memo[key]
    import zkgpu.parser as zp
    import zkgpu.synthetic_bytecode as sb
    shape = sb.load_shape()
    pid = sb.PARSERS.index(name)
    ext = pid >= 3
    ops, args = sb.generate(name, seed=1)
    secs = sb.sections(shape)
    prog = zp.convert(pid, ops, args, secs, shape["n_bits"], shape["n_bits_ext"])
    rng = np.random.default_rng(0)
    assert zkgpu.zxp_jit_cached(prog, _rand(rng, (8, 3)), _rand(rng, 48), _rand(rng, (2048, 3))), \
        "compiled kernel not cached: run build() (tools/jit_prebuild.py)"
    dom = 1 << LOG_DOM
    rng = np.random.default_rng(4000 + pid)
    S = {sec: _rand(rng, (dom, w)) for sec, _, w in secs if (sec >= 5) == ext}
    const = _rand(rng, (dom, shape["n_const"]))
    chal, pub, evals = _rand(rng, (8, 3)), _rand(rng, 48), _rand(rng, (2048, 3))
    xdiv, xdivw = (_rand(rng, (dom, 3)), _rand(rng, (dom, 3))) if ext else (None, None)
    x = np.zeros(dom, np.uint64)
    oracle.lib().oc_powers(oracle._p(x), 7 if ext else 1, oracle.gl_w(LOG_DOM), dom)
    zh = np.array([pow((pow(7, dom >> 1, P) * pow(P - 1, i, P) - 1) % P, P - 2, P) for i in range(2)], np.uint64)
    off = {sec: o for sec, o, _ in secs}
    R = {sec: a.copy() for sec, a in S.items()}
    out = np.zeros((dom, 3), np.uint64)
    sh = shape["programs"][name]
    kw = {} if not ext else {"q": out} if name == "step42ns" else {"f": out}
    rc = oracle.parser_eval(pid, ops, args, [(off[sec], a.shape[1], a) for sec, a in R.items()], const, dom,
                            1 << (shape["n_bits_ext"] if ext else shape["n_bits"]), max(sh["ntemp1"], 8),
                            max(sh["ntemp3"], 4), chal, pub, evals, x, zh,
                            xdiv if ext else np.zeros((dom, 3), np.uint64),
                            xdivw if ext else np.zeros((dom, 3), np.uint64), **kw)
    assert rc == 0
    before, after = dict(S), dict(R)
    before[SEC_CONST_2NS if ext else SEC_CONST_N] = after[SEC_CONST_2NS if ext else SEC_CONST_N] = const
    if ext:
        osec = SEC_Q_2NS if name == "step42ns" else SEC_F_2NS
        before[osec], after[osec] = np.zeros((dom, 3), np.uint64), out
    stores = bc.stores_of(prog)
    assert stores and all(not np.array_equal(after[sec][:, c], before[sec][:, c]) for sec, c in stores)
    if name == "step3":
        assert max(stores.values()) == 1  # the shifted stores
    widths = {sec: a.shape[1] for sec, a in before.items()}
    _memo[key] = (prog, stores, bc.max_shift(prog), widths, before, after, (chal, pub, evals), xdiv, xdivw)
    return _memo[key]


@pytest.mark.parametrize("log_rows,jit", [(10, "2"), (11, "0")], ids=["4blocks-jit2", "2blocks-jit0"])
@pytest.mark.parametrize("name", ["step3", "step42ns", "step52ns"])
def test_zkevm_shaped_programs_in_blocks(oracle, zkgpu, monkeypatch, name, log_rows, jit):
    monkeypatch.setenv("ZKGPU_ZXP_JIT", jit)
    prog, stores, halo, widths, before, after, scal, xdiv, xdivw = _shaped_reference(oracle, zkgpu, name)
    ext = name != "step3"
    g = bc.Geom(LOG_DOM, log_rows, halo, 0)
    loaded = bc.split(before, g.log_domain, g.log_rows, g.halo, g.pad, g.guard)
    zkgpu.prof_reset()
    zkgpu.prof_enable(True)
    try:
        got = _run_blocks(zkgpu, prog, loaded, widths, g, ext, 1 if ext else 0, *scal, xdiv, xdivw)
    finally:
        zkgpu.prof_enable(False)
    ran = zkgpu.prof_kernels()
    if jit == "2":
        assert "k_zxp_eval" not in ran and any(k.startswith("k_zxp_jit") for k in ran), ran
        if name == "step42ns":  # segments: carried values through scratch columns of a block's ld
            assert "k_zxp_jit_s00" in ran and len([k for k in ran if k.startswith("k_zxp_jit_s")]) > 1, ran
    else:
        assert "k_zxp_eval" in ran and not [k for k in ran if k.startswith("k_zxp_jit")], ran
    _check_blocks(got, before, after, stores, widths, g)


# ---------------------------------------------------------------- c. refusals
def _tiny(read_shift, store_shift):
    p = bc.Program(0)
    p.op(bc.ADD, p.col(bc.SEC_TMP_N, 0, store_shift), p.col(bc.SEC_CM1_N, 0, read_shift), p.col(bc.SEC_CM1_N, 1))
    return p


REFUSALS = {"log_rows_above_log_domain": "domain too large", "read_at_shift_minus_1": "operand 1 .* invalid",
            "ld_short_of_a_shifted_store": "operand 0 .* invalid", "accepted": None}


@pytest.mark.parametrize("what", list(REFUSALS))
@pytest.mark.parametrize("jit", ["0", "2"])
def test_refusals_queue_nothing(zkgpu, monkeypatch, what, jit):
    """ZKGPU_ERR_ARG (-2) and the image is still the loaded one; "accepted" is
    the call the three refused ones each differ from in one argument"""
    import torch
    monkeypatch.setenv("ZKGPU_ZXP_JIT", jit)
    log_rows, log_domain, s = 6, 8, 2
    rows = 1 << log_rows
    prog = _tiny(0, s)  # operand 0: the column stored at shift s, operand 1: the first column read
    ld = rows + s  # enough for the store at shift s
    if what == "log_rows_above_log_domain":
        log_domain = log_rows - 1
    elif what == "read_at_shift_minus_1":
        prog = _tiny(-1, s)
    elif what == "ld_short_of_a_shifted_store":
        ld = rows + s - 1
    rng = np.random.default_rng(9)
    widths = {bc.SEC_CM1_N: 2, bc.SEC_TMP_N: 1}
    img = {sec: rng.integers(0, P, size=w * ld + bc.GUARD, dtype=np.uint64) for sec, w in widths.items()}
    dev = {sec: zkgpu.to_device(a) for sec, a in img.items()}

    def call():
        zkgpu.zxp_eval_block_dev(prog, {sec: (dev[sec], ld, w) for sec, w in widths.items()}, log_rows, log_domain,
                                 rng.integers(0, P, size=(8, 3), dtype=np.uint64), None, x_start=1)

    if REFUSALS[what]:
        with pytest.raises(zkgpu.ZkgpuError, match=r"zkgpu_zxp_eval_block_dev failed \(-2\): .*" + REFUSALS[what]):
            call()
    else:
        call()
        a = img[bc.SEC_CM1_N]
        img[bc.SEC_TMP_N][s:rows + s] = [(int(x) + int(y)) % P for x, y in zip(a[:rows], a[ld:ld + rows])]
    torch.cuda.synchronize()
    for sec in widths:
        assert np.array_equal(zkgpu.from_device(dev[sec]), img[sec])
