"""The f values a plookup's table does not hold: the pure-Python reference and
the case table of zkgpu_lookup_misses_dev (include/zkgpu.h) and of layer A of
the prover's trace audit (include/zkgpu_stark.h zkgpu_stark_audit).

A column is a (dim, n) uint64 array (dim 1 or 3, component c of row i at
[c, i]); a value is the canonical dim-tuple, so v and v + p are one value.
reference(f, t, max_vals) returns what the primitive writes, as (n_rows,
n_vals, list): the rows of f whose value no row of t holds, the distinct such
values, and the first max_vals of them as (first row in f, count in f), by
ascending row."""
from collections import Counter

import numpy as np

from multiset_cases import P, distinct_column, tuples

PAD = (2**64 - 1, 0)


def reference_tuples(tf, tt, max_vals):
    table = set(tt)
    count = Counter(tf)
    first = {}
    for i, v in enumerate(tf):
        first.setdefault(v, i)
    miss = sorted((i, count[v]) for v, i in first.items() if v not in table)
    return sum(c for _, c in miss), len(miss), miss[:max_vals]


def reference(f, t, max_vals):
    return reference_tuples(tuples(f), tuples(t), max_vals)


def brute_force(f, t, max_vals):
    """the same by a double loop over rows (tiny inputs: checks the reference)"""
    tf, tt = tuples(f), tuples(t)
    n_rows, seen, lst = 0, [], []
    for i, v in enumerate(tf):
        if any(v == w for w in tt):
            continue
        n_rows += 1
        if v in seen:
            continue
        seen.append(v)
        lst.append((i, sum(1 for x in tf if x == v)))
    return n_rows, len(seen), lst[:max_vals]


def out_words(ref, max_vals):
    """the reference as the primitive's 2 + 2 * max_vals output words"""
    n_rows, n_vals, lst = ref
    words = [n_rows, n_vals]
    for k in range(max_vals):
        words += list(lst[k] if k < len(lst) else PAD)
    return np.array(words, dtype=np.uint64)


# ---------------------------------------------------------------- cases
SIZES = (0, 1, 2, 255, 256, 257, 1000, 1024, 1025, 4097)
ABSENT = P - 2  # component 0 of a value no generated column holds (theirs are below 2^40)


class Case:
    def __init__(self, name, f, t, max_vals=16, same=False, expect=None):
        self.name, self.f, self.t, self.max_vals, self.same = name, f, t, max_vals, same
        self.expect = expect  # what the construction promises, before the cut to max_vals

    def reference(self):
        return reference(self.f, self.t, self.max_vals)


def lookup_column(rng, t, n):
    """n rows drawn from the rows of t (with repeats: a plookup's source column)"""
    return t[:, rng.integers(0, t.shape[1], size=n)]


def cases(n, dim, seed=0):
    """the cases of one size and dimension (those that need a larger size are left out at small n)"""
    rng = np.random.default_rng([seed, n, dim])
    out = []
    t = distinct_column(rng, n, dim)
    if n == 0:
        e = np.zeros((dim, 0), np.uint64)
        return [Case("empty_%d" % mv, e, e, max_vals=mv, expect=(0, 0, [])) for mv in (0, 16)]
    f = lookup_column(rng, t, n)
    absent = t[:, :1].copy()
    absent[0, 0] = np.uint64(ABSENT)
    out.append(Case("no_miss", f, t, expect=(0, 0, [])))
    out.append(Case("same_pointer", t, t, same=True, expect=(0, 0, [])))
    for tag, rows in (("row0", [0]), ("last", [n - 1]), ("row0_and_last", sorted({0, n - 1}))):
        g = f.copy()
        g[:, rows] = absent
        out.append(Case("miss_" + tag, g, t, expect=(len(rows), 1, [(rows[0], len(rows))])))
    # one missing value on rows either side of a workgroup (256) and a reduction-block (1024) boundary
    for edge in (256, 1024):
        if n > edge + 1:
            rows = [edge - 2, edge - 1, edge, edge + 1]
            g = f.copy()
            g[:, rows] = absent
            out.append(Case("straddle_%d" % edge, g, t, expect=(4, 1, [(edge - 2, 4)])))
    # every row missing: with one value, with n distinct values
    out.append(Case("all_rows_one_value", np.repeat(absent, n, axis=1), t, expect=(n, 1, [(0, n)])))
    other = distinct_column(rng, n, dim, lo=n)  # shares no value with t
    for mv in (0, 16, 4096):
        out.append(Case("all_rows_distinct_%d" % mv, other, t, max_vals=mv,
                        expect=(n, n, [(i, 1) for i in range(n)])))
    if n >= 40:
        # more distinct misses than max_vals, between rows that hit: 20 values, the k-th on k + 1 rows
        g = f.copy()
        rows = rng.permutation(n)[:20 * 21 // 2] if n >= 210 else None
        if rows is not None:
            lst, at = [], 0
            for k in range(20):
                mine = sorted(int(r) for r in rows[at:at + k + 1])
                at += k + 1
                g[:, mine] = other[:, k:k + 1]
                lst.append((mine[0], k + 1))
            out.append(Case("twenty_values", g, t, max_vals=16, expect=(210, 20, sorted(lst))))
    # canonicalisation: v < 2^32 - 1 against v + p (v + p < 2^64), on either side; the rows [1, n)
    # of f hold table values, row 0 one that is absent in both spellings
    small = np.zeros((dim, n), np.uint64)
    small[:] = rng.permutation(n).astype(np.uint64)[None, :]
    for c in range(dim):
        small[c] = np.roll(small[c], c)
    fs = lookup_column(rng, small, n)
    fs[:, 0] = np.uint64(n + 5)
    exp = (1, 1, [(0, 1)])
    out.append(Case("canonical_f", fs + np.uint64(P), small, expect=exp))
    out.append(Case("canonical_t", fs, small + np.uint64(P), expect=exp))
    if dim == 3:
        g = f.copy()
        r = n // 2
        g[2, r] = (g[2, r] + np.uint64(1)) % np.uint64(P)  # (the other components random: no row of t has it)
        out.append(Case("last_component", g, t, expect=(1, 1, [(r, 1)])))
    return out
