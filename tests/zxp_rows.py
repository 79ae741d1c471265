"""Checker of the prover's probe (include/zkgpu_stark.h zkgpu_stark_probe_*):
the ZXP source programs (include/zkgpu_zxp.h) re-evaluated on sampled rows.

eval_rows    one program on the rows its before-records reach (numpy object
             arrays of Python ints: exact, no section larger than the records)
check_probe  every program point of a probe: evaluate from the before-records
             and scalars, compare every stored column with the after-record
oracle_probe the same records from oracle.stark_prover.OracleStark
plan         the record list a probe has (the rule of host/starks_diag.cpp Probe::set)

Conventions as oracle/stark.c zxp_run: temporaries are zero at the start of a
row, F_p^3 (+/-) F_p touches component 0, a store canonicalises, a base value
stored to an F_p^3 destination zeroes components 1 and 2.
"""
import numpy as np

P = 0xFFFFFFFF00000001
TMP1, TMP3, COL, COL3, LIT, CHAL, PUB, X, EVAL, XDIV, XDIVW, ZI = range(12)
ADD, SUB, MUL, COPY = range(4)
SEC_COUNT = 12
SEC_CM2_N, SEC_CM3_N, SEC_CM1_2NS, SEC_CM4_2NS = 1, 2, 5, 8
SCALARS = 0xFFFFFFFF
STEP2, H1H2, STEP3PREV, Z, STEP3, STEP42NS, QSPLIT, STEP52NS = range(8)
PROGRAM_POINTS = {STEP2: "step2", STEP3PREV: "step3prev", STEP3: "step3", STEP42NS: "step42ns", STEP52NS: "step52ns"}
POINT_NAMES = ["step2", "h1h2", "step3prev", "z", "step3", "step42ns", "qsplit", "step52ns"]
W32 = 7277203076849721926


def gl_w(n):
    w = W32
    for _ in range(n, 32):
        w = w * w % P
    return w


def f3_mul(a, b):
    """F_p[x] / (x^3 - x - 1); components are ints or object arrays"""
    a0, a1, a2 = a
    b0, b1, b2 = b
    t = a1 * b2 + a2 * b1
    u = a2 * b2
    return ((a0 * b0 + t) % P, (a0 * b1 + a1 * b0 + t + u) % P, (a0 * b2 + a1 * b1 + a2 * b0 + u) % P)


def f3_inv(a):
    """a^(p^3 - 2), scalar"""
    r, base, e = (1, 0, 0), tuple(int(v) % P for v in a), P ** 3 - 2
    while e:
        if e & 1:
            r = f3_mul(r, base)
        base = f3_mul(base, base)
        e >>= 1
    return r


def section_widths(inst):
    return [inst.n_cm1, inst.n_cm2, inst.n_cm3, inst.n_tmp, inst.n_const, inst.n_cm1, inst.n_cm2, inst.n_cm3,
            inst.n_cm4, inst.n_const, 3, 3]


def _shift(c):
    c = int(c)
    return c - (1 << 32) if c >= 1 << 31 else c


def program_sections(prog):
    """(reads, stores, shifts): the sections a program's COL / COL3 operands
    read and store to, and per section every row shift used with it plus 0"""
    ins, opn = prog.arrays()
    reads, stores, shifts = set(), set(), {}
    for op, dst, a, b in ins.tolist():
        uses =[(a, False), (dst, True)] + ([(b, False)] if op != COPY else [])
        for k, store in uses:
            kind, sec, _, c = opn[k].tolist()
            if kind not in (COL, COL3):
                continue
            (stores if store else reads).add(sec)
            shifts.setdefault(sec, {0}).add(_shift(c))
    return reads, stores, shifts


def plan(inst, rows_n, rows_ext):
    """[(point, after, section, ncols, rows)] of a probe of these sampled rows"""
    base = [np.unique(np.asarray(rows_n, np.uint64)), np.unique(np.asarray(rows_ext, np.uint64))]
    widths = section_widths(inst)
    n_scal = 24 + 3 * len(inst.evmap)
    out = []
    for point in range(8):
        ext = point >= STEP42NS
        dom = 1 << (inst.n_bits_ext if ext else inst.n_bits)
        if point in PROGRAM_POINTS:
            prog = inst.programs.get(PROGRAM_POINTS[point])
            if point == STEP3 and (prog is None or not prog.instr):
                continue
        elif point == H1H2 and not inst.pu:
            continue
        out.append((point, 0, SCALARS, n_scal, np.zeros(1, np.uint64)))
        if point not in PROGRAM_POINTS:
            sec = {H1H2: SEC_CM2_N, Z: SEC_CM3_N, QSPLIT: SEC_CM4_2NS}[point]
            out.append((point, 1, sec, widths[sec], base[ext]))
            continue
        if prog is None or not prog.instr:
            continue
        reads, stores, shifts = program_sections(prog)
        for sec in reads | stores:
            if (sec >= SEC_CM1_2NS) != ext:
                raise ValueError("%s uses section %d of the other domain" % (PROGRAM_POINTS[point], sec))
        rows = {}
        for sec in reads | stores:
            r = {(int(x) + s) % dom for x in base[ext] for s in shifts[sec]}
            rows[sec] = np.array(sorted(r), np.uint64)
        for after, secs in ((0, reads), (1, stores)):
            for sec in sorted(secs):
                out.append((point, after, sec, widths[sec], rows[sec]))
    return out


def eval_rows(prog, dom_bits, ext, eb, records_before, scalars, publics, rows=None, xdiv=None, xdivw=None):
    """Evaluate a ZXP source program on sampled rows.

    records_before: {section: (rows, vals (n_rows, ncols))}; scalars:
    challenges[24] then evals; rows: the rows to evaluate (default: every row
    whose reads the records cover); xdiv / xdivw: (rows, vals (n_rows, 3))
    records of the caller's x/(x - xi), x/(x - w xi) arrays, read in place of
    the values derived from challenge 7.  Returns {(section, column): (rows
    written, values)}: a store at shift s writes row (r + s) mod dom.
    Raises ValueError on a shifted read of a column the program itself stores
    (at another shift than the store's) and KeyError on a row the records lack."""
    ins, opn = prog.arrays()
    ins, opn = ins.tolist(), opn.tolist()
    dom = 1 << dom_bits
    scal = [int(v) for v in np.asarray(scalars).ravel()]
    ch, evals = scal[:24], scal[24:]
    pub = [int(v) for v in np.asarray(publics).ravel()]
    recs = {sec: (np.asarray(r, np.uint64).astype(np.int64), np.asarray(v)) for sec, (r, v) in records_before.items()}
    # stores: column -> shift (one shift per stored column)
    store_shift = {}
    for op, dst, a, b in ins:
        kind, sec, col, c = opn[dst]
        if kind in (COL, COL3):
            for k in range(3 if kind == COL3 else 1):
                if store_shift.setdefault((sec, col + k), _shift(c)) != _shift(c):
                    raise ValueError("column %d of section %d is stored at two shifts" % (col + k, sec))
    if rows is None:
        cand = None
        for op, dst, a, b in ins:
            for k in (a,) if op == COPY else (a, b):
                kind, sec, col, c = opn[k]
                if kind in (COL, COL3) and sec in recs:
                    ok = set(((recs[sec][0] - _shift(c)) % dom).tolist())
                    cand = ok if cand is None else cand & ok
        if cand is None:
            raise ValueError("eval_rows: no column read to infer the rows from; pass rows")
        rows = sorted(cand)
    R = np.array([int(r) for r in rows], dtype=object)
    nR = len(R)
    zero = np.zeros(nR, dtype=object)
    nb = dom_bits - eb if ext else dom_bits
    w_dom, w_n = gl_w(dom_bits), gl_w(nb)
    x = np.array([(7 if ext else 1) * pow(w_dom, int(r), P) % P for r in R], dtype=object)
    lazy = {}
    for kind, rec in ((XDIV, xdiv), (XDIVW, xdivw)):
        if rec is not None:
            rr, vals = np.asarray(rec[0], np.uint64).astype(np.int64), np.asarray(rec[1])
            idx = np.searchsorted(rr, R.astype(np.int64))
            if (idx >= rr.size).any() or (rr[np.minimum(idx, rr.size - 1)] != R.astype(np.int64)).any():
                raise KeyError("a row is not in the xdiv record")
            lazy[kind] = tuple(vals[idx, k].astype(object) for k in range(3))

    def special(kind):
        if kind not in lazy:
            if not ext:
                raise ValueError("ZXP_XDIV / XDIVW / ZI on the n domain")
            if kind == ZI:
                N = 1 << nb
                lazy[kind] = np.array([pow((pow(int(v), N, P) - 1) % P, P - 2, P) for v in x], dtype=object)
            else:
                xi = ch[21:24]
                if kind == XDIVW:
                    xi = [v * w_n % P for v in xi]
                comps = [[], [], []]
                for v in x:
                    i = f3_inv(((int(v) - xi[0]) % P, (-xi[1]) % P, (-xi[2]) % P))
                    for k in range(3):
                        comps[k].append(i[k] * int(v) % P)
                lazy[kind] = tuple(np.array(c, dtype=object) for c in comps)
        return lazy[kind]

    t1, t3, stored = {}, {}, {}

    def column(sec, col, sh):
        if (sec, col) in store_shift:
            if store_shift[(sec, col)] != sh:
                raise ValueError("shifted read (shift %d) of column %d of section %d, which the program stores at "
                                 "shift %d" % (sh, col, sec, store_shift[(sec, col)]))
            if (sec, col) in stored:
                return stored[(sec, col)]
        if sec not in recs:
            raise KeyError("no before-record of section %d" % sec)
        rr, vals = recs[sec]
        want = ((R + sh) % dom).astype(np.int64)
        idx = np.searchsorted(rr, want)
        if (idx >= rr.size).any() or (rr[np.minimum(idx, rr.size - 1)] != want).any():
            raise KeyError("section %d: a row at shift %d is not in the before-record" % (sec, sh))
        return vals[idx, col].astype(object)

    def load(k):
        kind, a, b, c = opn[k]
        if kind == TMP1:
            return 1, (t1.get(a, zero),)
        if kind == TMP3:
            return 3, t3.get(a, (zero, zero, zero))
        if kind == COL:
            return 1, (column(a, b, _shift(c)),)
        if kind == COL3:
            return 3, tuple(column(a, b + k3, _shift(c)) for k3 in range(3))
        if kind == LIT:
            return 1, ((a | (b << 32)) % P,)
        if kind == CHAL:
            return 3, tuple(ch[3 * a:3 * a + 3])
        if kind == PUB:
            return 1, (pub[a],)
        if kind == X:
            return 1, (x,)
        if kind == EVAL:
            return 3, tuple(evals[3 * a:3 * a + 3])
        if kind in (XDIV, XDIVW):
            return 3, special(kind)
        if kind == ZI:
            return 1, (special(ZI),)
        raise ValueError("operand kind %d" % kind)

    for op, dst, a, b in ins:
        da, va = load(a)
        if op == COPY:
            d, v = da, va
        else:
            db, vb = load(b)
            d = max(da, db)
            if op == MUL:
                if da == 3 and db == 3:
                    v = f3_mul(va, vb)
                elif da == 3:
                    v = tuple(c * vb[0] % P for c in va)
                elif db == 3:
                    v = tuple(c * va[0] % P for c in vb)
                else:
                    v = (va[0] * vb[0] % P,)
            else:
                pa = va + (0, 0) if da == 1 else va
                pb = vb + (0, 0) if db == 1 else vb
                v = tuple(((p + q) if op == ADD else (p - q)) % P for p, q in zip(pa, pb))[:d]
        kind, sa, sb, sc = opn[dst]
        if kind == TMP1:
            t1[sa] = v[0] % P
        elif kind == TMP3:
            t3[sa] = tuple(c % P for c in v) if d == 3 else (v[0] % P, 0, 0)
        elif kind in (COL, COL3):
            comps = (v[0],) if kind == COL else (tuple(v) if d == 3 else (v[0], 0, 0))
            for k3, c in enumerate(comps):
                stored[(sa, sb + k3)] = (zero + c) % P
        else:
            raise ValueError("destination kind %d" % kind)
    out = {}
    for (sec, col), v in stored.items():
        target = ((R + store_shift[(sec, col)]) % dom).astype(np.uint64)
        out[(sec, col)] = (target, v.astype(np.uint64))
    return out


def split_probe(probe):
    """{point: {"scalars": vals, "before": {sec: (rows, vals)}, "after": {...}}}"""
    out = {}
    for point, after, sec, rows, vals in probe:
        d = out.setdefault(int(point), {"scalars": None, "before": {}, "after": {}})
        if sec == SCALARS:
            d["scalars"] = np.asarray(vals).ravel()
        else:
            d["after" if after else "before"][int(sec)] = (np.asarray(rows), np.asarray(vals))
    return out


def check_probe(inst, probe, publics, stats=None):
    """Re-evaluate every program point of a probe ([(point, after, section,
    rows, vals)], GpuStark.probe()) from its before-records and scalars and
    compare every stored column with the after-record on every row both have.
    Returns the mismatches [(point, section, row, column)].  stats (a dict):
    filled with {point: {"rows", "cols", "nonzero"}} of what was compared."""
    bad = []
    by_point = split_probe(probe)
    for point, name in sorted(PROGRAM_POINTS.items()):
        prog = inst.programs.get(name)
        d = by_point.get(point)
        if d is None or prog is None or not prog.instr:
            continue
        ext = point >= STEP42NS
        got = eval_rows(prog, inst.n_bits_ext if ext else inst.n_bits, ext, inst.blowup_bits, d["before"],
                        d["scalars"], publics)
        st = {"rows": 0, "cols": 0, "nonzero": False}
        for (sec, col), (target, vals) in sorted(got.items()):
            if sec not in d["after"]:
                raise ValueError("%s stores to section %d, the probe has no after-record of it" % (name, sec))
            rr, av = d["after"][sec]
            rr = rr.astype(np.int64)
            t = target.astype(np.int64)
            idx = np.minimum(np.searchsorted(rr, t), max(rr.size - 1, 0))
            have = rr[idx] == t if rr.size else np.zeros(t.size, bool)
            ref = av[idx[have], col].astype(np.uint64)
            mine = vals[have]
            st["rows"] = max(st["rows"], int(have.sum()))
            st["cols"] += 1
            st["nonzero"] = st["nonzero"] or bool(ref.any())
            for r in t[have][ref != mine].tolist():
                bad.append((point, sec, int(r), col))
        if stats is not None:
            stats[point] = st
    return bad


def oracle_probe(ostark, rows_n, rows_ext):
    """(records, proof): one OracleStark proof with the probe's records
    ([(point, after, section, rows, vals)], as GpuStark.probe()) taken around
    every OracleStark.run; the H1H2 / Z / quotient-split after-records from
    the sections where nothing has written them since (cm2_n before
    step3prev; cm3_n before step3, or at the end without one; cm4 at the end:
    each of those columns is written once)."""
    inst = ostark.inst
    pl = plan(inst, rows_n, rows_ext)
    n_ev = len(inst.evmap)
    point_of = {id(inst.programs[name]): pt for pt, name in PROGRAM_POINTS.items() if name in inst.programs}
    vals, scal = {}, {}

    def take(point, after):
        for pt, af, sec, ncols, rows in pl:
            if pt == point and af == after and sec != SCALARS and (pt, af, sec) not in vals:
                vals[(pt, af, sec)] = ostark.S[sec][rows.astype(np.int64)][:, :ncols].copy()

    def scalars(ch, evals):
        s = np.zeros(24 + 3 * n_ev, np.uint64)
        s[:24] = np.asarray(ch, np.uint64).ravel()
        ev = np.asarray(evals, np.uint64).ravel()
        if n_ev and ev.size == 3 * n_ev:
            s[24:] = ev
        return s

    orig = ostark.run

    def run(prog, challenges, evals, xdiv=None, xdivw=None):
        point = point_of.get(id(prog))
        if point is None:
            return orig(prog, challenges, evals, xdiv, xdivw)
        scal[point] = scalars(challenges, evals)
        if point == STEP3PREV:
            take(H1H2, 1)
        if point == STEP3:
            take(Z, 1)
        take(point, 0)
        orig(prog, challenges, evals, xdiv, xdivw)
        take(point, 1)

    ostark.run = run
    try:
        proof = ostark.prove()
    finally:
        del ostark.run
    take(Z, 1)
    take(QSPLIT, 1)
    scal[H1H2], scal[Z], scal[QSPLIT] = scal[STEP2], scal[STEP3PREV], scal[STEP42NS]
    out = []
    for pt, af, sec, ncols, rows in pl:
        v = scal[pt].reshape(1, -1) if sec == SCALARS else vals[(pt, af, sec)]
        out.append((pt, af, sec, rows.copy(), v))
    return out, proof


def assert_same_probe(got, want):
    """record by record: point order, sections, row lists, values"""
    assert [(int(p), int(a), int(s)) for p, a, s, _, _ in got] == [(int(p), int(a), int(s)) for p, a, s, _, _ in want]
    for (p, a, s, r0, v0), (_, _, _, r1, v1) in zip(got, want):
        where = "%s %s section %s" % (POINT_NAMES[p], "after" if a else "before", "scalars" if s == SCALARS else s)
        assert np.array_equal(np.asarray(r0, np.uint64), np.asarray(r1, np.uint64)), where + ": rows"
        v0, v1 = np.asarray(v0, np.uint64), np.asarray(v1, np.uint64)
        assert v0.shape == v1.shape, where + ": shape %s / %s" % (v0.shape, v1.shape)
        if not np.array_equal(v0, v1):
            i, c = np.argwhere(v0 != v1)[0]
            raise AssertionError("%s: first difference at row %d column %d" % (where, int(np.asarray(r0)[i]), c))
