"""The cells a connection check leaves unequal: the pure-Python reference and
the case table of zkgpu_conn_breaks_dev (include/zkgpu.h) and of the prover's
zkgpu_stark_conn_check (include/zkgpu_stark.h).

On the trace domain of n = 2^n_bits rows with generator w, cell (j, r) -- the
number j n + r -- has the identity ks[j] w^r, and S[i][r] holds the identity of
the cell that (i, r) is wired to.  a and s are (k, n) uint64 arrays; v and
v + p are one value, S values too.  reference(a, s, ks, n_bits, max_vals)
returns what the primitive writes, as ((n_broken, n_foreign, n_untargeted),
breaks, foreign): the first max_vals broken cells as (cell, target, value,
value at target) and the first max_vals foreign cells as (cell, S value), both
ascending by cell, values canonical."""
import numpy as np

P = 0xFFFFFFFF00000001
W32 = 7277203076849721926  # a generator of the subgroup of order 2^32
NONE = 2**64 - 1
SHAPES = ((0, 1), (3, 1), (5, 2), (5, 3), (6, 12), (8, 3), (10, 2))


def omega(n_bits):
    w = W32
    for _ in range(n_bits, 32):
        w = w * w % P
    return w


def default_ks(k):
    return [pow(12, i, P) for i in range(k)]


def identities(ks, n_bits):
    """identity of every cell, by cell number"""
    w, ids = omega(n_bits), []
    for kj in ks:
        x = kj % P
        for _ in range(1 << n_bits):
            ids.append(x)
            x = x * w % P
    return ids


def ks_collision(ks, n_bits):
    """None, or what zkgpu_conn_breaks_dev says when it refuses ks"""
    seen = []
    for j, kj in enumerate(ks):
        if kj % P == 0:
            return "conn_breaks: ks[%d] is zero" % j
        y = pow(kj, 1 << n_bits, P)
        if y in seen:
            return "conn_breaks: the cosets of ks[%d] and ks[%d] collide" % (seen.index(y), j)
        seen.append(y)
    return None


def reference(a, s, ks, n_bits, max_vals):
    k, n = a.shape
    assert n == 1 << n_bits and s.shape == a.shape and ks_collision(ks, n_bits) is None
    cell_of = {v: c for c, v in enumerate(identities(ks, n_bits))}
    assert len(cell_of) == k * n
    va = [int(v) % P for v in a.ravel()]
    vs = [int(v) % P for v in s.ravel()]
    named, breaks, foreign = set(), [], []
    for c in range(k * n):
        t = cell_of.get(vs[c])
        if t is None:
            foreign.append((c, vs[c]))
            continue
        named.add(t)
        if va[c] != va[t]:
            breaks.append((c, t, va[c], va[t]))
    return (len(breaks), len(foreign), k * n - len(named)), breaks[:max_vals], foreign[:max_vals]


def out_words(ref, max_vals):
    """the reference as the primitive's 3 + 6 * max_vals output words"""
    counts, breaks, foreign = ref
    words = list(counts)
    for e in range(max_vals):
        words += list(breaks[e]) if e < len(breaks) else [NONE, 0, 0, 0]
    for e in range(max_vals):
        words += list(foreign[e]) if e < len(foreign) else [NONE, 0]
    return np.array(words, dtype=np.uint64)


def closes(a, s, ks, n_bits, beta, gamma):
    """does the grand product close: prod (a + beta ks x + gamma) == prod (a + beta S + gamma)"""
    ids = identities(ks, n_bits)
    num = den = 1
    for c, (va, vs) in enumerate(zip(a.ravel(), s.ravel())):
        num = num * ((int(va) + beta * ids[c] + gamma) % P) % P
        den = den * ((int(va) + beta * int(vs) + gamma) % P) % P
    return num == den


# ---------------------------------------------------------------- cases
class Case:
    def __init__(self, name, a, s, ks, n_bits, max_vals=16, default_ks=True, expect=None):
        self.name, self.a, self.s, self.n_bits, self.max_vals = name, a, s, n_bits, max_vals
        self.ks = list(ks)
        self.ks_arg = None if default_ks else self.ks  # what the call is given
        self.expect = expect  # the counts the construction promises

    def reference(self):
        return reference(self.a, self.s, self.ks, self.n_bits, self.max_vals)


def wiring(ids, perm, shape):
    """S for the wiring cell c -> perm[c]"""
    return np.array([ids[t] for t in perm], dtype=np.uint64).reshape(shape)


def cycle_values(rng, perm):
    """one random value per cycle of perm"""
    val = np.zeros(len(perm), np.uint64)
    seen = np.zeros(len(perm), bool)
    for c in range(len(perm)):
        if seen[c]:
            continue
        v = rng.integers(0, P, dtype=np.uint64)
        while not seen[c]:
            seen[c], val[c] = True, v
            c = perm[c]
    return val


def one_cycle(rng, cells):
    order = rng.permutation(cells)
    perm = np.zeros(cells, np.int64)
    perm[order] = np.roll(order, -1)
    return perm


def cases(n_bits, k, seed=0):
    rng = np.random.default_rng([seed, n_bits, k])
    n, cells, shape = 1 << n_bits, k << n_bits, (k, 1 << n_bits)
    ks = default_ks(k)
    ids = identities(ks, n_bits)
    out = []

    def add(name, a, s, expect, **kw):
        kw.setdefault("ks", ks)
        out.append(Case(name, np.asarray(a, np.uint64).reshape(shape), np.asarray(s, np.uint64).reshape(shape),
                        n_bits=n_bits, expect=expect, **kw))

    perm = rng.permutation(cells)
    val = cycle_values(rng, perm)
    add("clean_random", val, wiring(ids, perm, shape), (0, 0, 0))
    ident = np.arange(cells)
    add("identity", rng.integers(0, P, size=cells, dtype=np.uint64), wiring(ids, ident, shape), (0, 0, 0))
    cyc = one_cycle(rng, cells)
    same = np.full(cells, 77, np.uint64)
    add("one_cycle", same, wiring(ids, cyc, shape), (0, 0, 0))
    # a fixed point may hold anything
    fp = int(rng.integers(0, cells))
    rest = np.array([c for c in range(cells) if c != fp], np.int64)
    pf = np.arange(cells)
    pf[rest] = rest[rng.permutation(len(rest))] if len(rest) else rest
    vf = cycle_values(rng, pf)
    vf[fp] = (vf[fp] + np.uint64(1)) % np.uint64(P)
    add("fixed_point_off", vf, wiring(ids, pf, shape), (0, 0, 0))
    # S with a value that is no identity: 0, and a value of a coset that ks does not hold
    other_coset = pow(12, k, P) * pow(omega(n_bits), 3, P) % P
    for tag, bad in (("zero", 0), ("coset", other_coset), ("zero_plus_p", P)):
        for where in sorted({0, cells - 1}):
            s = wiring(ids, cyc, shape).ravel()
            s[where] = np.uint64(bad)
            add("foreign_%s_at_%d" % (tag, where), same, s, (0, 1, 1))
    # canonicalisation: values v + p, and the identity 1 of cell 0 spelled 1 + p
    small = cycle_values(np.random.default_rng([seed, 1]), perm) % np.uint64(2**32 - 1)
    s = wiring(ids, perm, shape).ravel()
    lift = rng.integers(0, 2, size=cells, dtype=np.uint64) * np.uint64(P)
    lift[0] = np.uint64(P)
    s[int(np.nonzero(perm == 0)[0][0])] = np.uint64(1 + P)
    add("canonical", small + lift, s, (0, 0, 0))
    if cells >= 2:
        # one cell off inside a cycle: the cell and the cell wired to it, both naming it
        for tag, c in (("first", 0), ("last", cells - 1), ("middle", cells // 2)):
            v = same.copy()
            v[c] += np.uint64(1)
            add("one_off_" + tag, v, wiring(ids, cyc, shape), (2, 0, 0))
        # every link broken: more than max_vals
        for mv in (0, 1, 16):
            add("all_broken_%d" % mv, np.arange(cells, dtype=np.uint64) + np.uint64(P - 3), wiring(ids, cyc, shape),
                (cells, 0, 0), max_vals=mv)
        # two cells name one target
        s = wiring(ids, cyc, shape).ravel()
        s[cells - 1] = s[0]
        add("duplicate_target", same, s, (0, 0, 1))
        # (cell cells - 1 is now wired to cyc[0]: to itself, and so unbroken, if that is cells - 1)
        add("duplicate_target_broken", np.arange(cells, dtype=np.uint64), s,
            (cells - (cyc[0] == cells - 1), 0, 1), max_vals=16)
    # shifts of the caller's
    ks2 = [5 * pow(7, i, P) % P for i in range(k)]
    ids2 = identities(ks2, n_bits)
    add("own_ks_clean", val, wiring(ids2, perm, shape), (0, 0, 0), ks=ks2, default_ks=False)
    if cells >= 2:
        v = same.copy()
        v[cells - 1] += np.uint64(1)
        add("own_ks_one_off", v, wiring(ids2, cyc, shape), (2, 0, 0), ks=ks2, default_ks=False)
        # the default wiring read with other shifts: (almost) every S value is foreign
        add("own_ks_mismatch", same, wiring(ids, cyc, shape), None, ks=ks2, default_ks=False)
    return out
