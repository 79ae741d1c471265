"""The row-block model (tests/block_cases.py) checked without a GPU.

The row-list interpreter of tests/zxp_rows.py stands in for the device: it
evaluates rows [row0, row0 + 2^log_rows) of the whole domain from the rows a
block holds (its own and the halo), and the results are laid out as a block
call leaves them.  The assertions tests/test_gpu_zxp_eval_block.py runs on the
device's images then pass for every case, block size, pad and block, and
the blocks recompose to the oracle's whole-domain oc_zxp_eval bit for bit.
Three wrong stand-ins -- one that wraps inside the block, one that starts x at
the coset shift in every block, one that drops the halo part of a shifted
store -- each fail them.
"""
import numpy as np
import pytest

import block_cases as bc
import zxp_rows as zr

_memo = {}


def _reference(oracle, name):
    """(case, inputs, the oracle's whole-domain sections), once per case"""
    if name not in _memo:
        case = bc.CASES[name]()
        inp = bc.Inputs(case, seed=sum(map(ord, name)))
        _memo[name] = (case, inp, bc.oracle_whole(oracle, case, inp))
    return _memo[name]


def _block_values(case, inp, g, b, fault):
    """{(section, column): values of rows row0 .. row0 + 2^log_rows - 1} from
    the rows block b holds, by zr.eval_rows; fault: None, "wrap" (the halo rows
    hold the block's own first rows) or "x7" (x starts at the coset shift: the
    block evaluated as if it were block 0)."""
    R, row0, N = g.rows, g.row0(b), g.N
    have = (row0 + np.arange(R + g.halo)) % N
    vals = {sec: a[have] for sec, a in inp.S_canon.items()}
    if fault == "wrap":
        for a in vals.values():
            a[R:] = a[:g.halo]
    labels = have
    rows = row0 + np.arange(R)
    if fault == "x7" and g.nblocks > 1:
        labels = np.arange(R + g.halo)
        rows = np.arange(R)
    # (a single block's halo rows are its own first rows: one record of each)
    n_lab = R + g.halo if g.nblocks > 1 else R
    order = np.argsort(labels[:n_lab])
    recs = {sec: (labels[:n_lab][order], a[:n_lab][order]) for sec, a in vals.items()}
    xrec = [(rows, x[row0:row0 + R]) if case.ext else None for x in (inp.xdiv, inp.xdivw)]
    out = zr.eval_rows(case.prog, case.log_domain, case.ext, case.eb, recs,
                       np.concatenate([inp.chal.ravel(), inp.evals.ravel()]), inp.pub, rows=rows, xdiv=xrec[0],
                       xdivw=xrec[1])
    return {k: v for k, (_target, v) in out.items()}


def _standin(case, inp, g, loaded, fault=None):
    """the images all blocks' calls leave, per block, from the loaded ones"""
    key = (case.name, g.log_rows, fault if fault in ("wrap", "x7") else None)
    if key not in _memo:
        _memo[key] = [_block_values(case, inp, g, b, key[2]) for b in range(g.nblocks)]
    out = []
    for b, blk in enumerate(loaded):
        blk = {sec: img.copy() for sec, img in blk.items()}
        for (sec, col), v in _memo[key][b].items():
            s = case.stores[(sec, col)]
            r = s + np.arange(g.rows)
            if fault == "wrap":
                r %= g.rows
            if fault == "drop_halo":
                v, r = v[r < g.rows], r[r < g.rows]
            g.columns(blk[sec], case.widths[sec])[col, r] = v
        out.append(blk)
    return out


def _check(oracle, name, log_rows, pad, fault=None):
    case, inp, after = _reference(oracle, name)
    g = bc.Geom(case.log_domain, log_rows, case.halo, pad)
    loaded = bc.split(inp.S, g.log_domain, g.log_rows, g.halo, g.pad, g.guard)
    want = bc.expected(inp.S, after, case.stores, g)
    got = _standin(case, inp, g, loaded, fault)
    for b in range(g.nblocks):
        bc.assert_block(got[b], want[b], case.widths, g, b)
    bc.assert_recomposed(got, case.stores, after, case.widths, g)


def _cases():
    return [pytest.param(n, lr, pad, id="%s-r%d-pad%d" % (n, lr, pad)) for n in bc.CASES for lr in bc.LOG_ROWS[n]
            for pad in bc.PADS]


@pytest.mark.parametrize("name,log_rows,pad", _cases())
def test_standin_passes_and_recomposes(oracle, name, log_rows, pad):
    _check(oracle, name, log_rows, pad)


def test_programs_and_inputs_are_what_the_cases_promise(oracle):
    for name in bc.CASES:
        case, inp, after = _reference(oracle, name)
        assert len(case.prog.instr) < 150
        stored_cols = set(case.stores)
        ins, opn = case.prog.arrays()
        for op, _dst, a, b in ins.tolist():  # no stored cell is read
            for k in (a,) if op == bc.COPY else (a, b):
                kind, sec, col, _c = opn[k].tolist()
                if kind in (bc.COL, bc.COL3):
                    assert not {(sec, col + j) for j in range(3 if kind == bc.COL3 else 1)} & stored_cols
        for (sec, col) in case.stores:  # the program wrote, and wrote canonical words
            assert not np.array_equal(after[sec][:, col], inp.S_canon[sec][:, col])
            assert (after[sec][:, col] < np.uint64(bc.P)).all()
        assert any((a >= np.uint64(bc.P)).any() for a in inp.S.values())  # lazy words are in play
    assert sorted(set(bc.stage().stores.values())) == [0, 1, 2]
    assert bc.stage().halo == 2 and bc.quotient(2).halo == 4 and bc.fri().halo == 0


def test_split_poisons_pad_and_guard_and_wraps_the_last_halo():
    S = {0: np.arange(32, dtype=np.uint64).reshape(16, 2)}
    blocks = bc.split(S, 4, 2, 1, 2, 3)
    g = bc.Geom(4, 2, 1, 2, 3)
    assert len(blocks) == 4 and blocks[0][0].size == 2 * 7 + 3
    last = g.columns(blocks[3][0], 2)
    assert last[0].tolist() == [24, 26, 28, 30, 0, bc.POISON, bc.POISON]
    assert blocks[3][0][-3:].tolist() == [bc.POISON] * 3
    # a block left out, or one twice: recompose notices
    exp = bc.expected(S, S, {(0, 1): 1}, g)
    bc.assert_recomposed(exp, {(0, 1): 1}, S, {0: 2}, g)
    with pytest.raises(AssertionError, match="comes from"):
        bc.recompose(exp[:3], {(0, 1): 1}, {0: 2}, g)


def _fault_cases():
    out = []
    for n in bc.CASES:
        for lr in bc.LOG_ROWS[n]:
            whole = lr == bc.LOG_ROWS[n][0]  # W = 1
            if n == "stage" or (n.startswith("quotient") and not whole):
                out.append(("wrap", n, lr))  # (quotient at W = 1: wrapping in the block is wrapping in the domain)
            if n != "fri" and not whole:
                out.append(("x7", n, lr))  # the programs that read X, where a block other than the first exists
            if n == "stage":
                out.append(("drop_halo", n, lr))  # the program with shifted stores
    return [pytest.param(*c, id="-".join(map(str, c))) for c in out]


@pytest.mark.parametrize("fault,name,log_rows", _fault_cases())
def test_injected_errors_fail_the_assertions(oracle, fault, name, log_rows):
    with pytest.raises(AssertionError, match="differ"):
        _check(oracle, name, log_rows, 0, fault)
