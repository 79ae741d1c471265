"""Multiset comparison of two columns: the pure-Python reference and the case
table of zkgpu_multiset_diff_dev (include/zkgpu.h) and of the prover's
calculateZ diagnosis (include/zkgpu_stark.h zkgpu_z_diag).

A column is a (dim, n) uint64 array (dim 1 or 3, component c of row i at
[c, i]); a value is the canonical dim-tuple, so v and v + p are one value.
reference(a, b, max_vals) returns what the primitive writes, as
(n_a, list_a, n_b, list_b): per side the number of distinct values that occur
on that side with unequal counts and the first max_vals of them as (first row
on that side, count in a, count in b), by ascending row."""
from collections import Counter

import numpy as np

P = 0xFFFFFFFF00000001
PAD = (2**64 - 1, 0, 0)


def tuples(col):
    col = np.asarray(col, dtype=np.uint64)
    if col.ndim == 1:
        col = col.reshape(1, -1)
    canon = col % np.uint64(P)
    return [tuple(int(x) for x in canon[:, i]) for i in range(canon.shape[1])]


def reference_tuples(ta, tb, max_vals):
    ca, cb = Counter(ta), Counter(tb)
    out = []
    for side in (ta, tb):
        first = {}
        for i, v in enumerate(side):
            first.setdefault(v, i)
        bad = sorted((i, ca[v], cb[v]) for v, i in first.items() if ca[v] != cb[v])
        out += [len(bad), bad[:max_vals]]
    return tuple(out)


def reference(a, b, max_vals):
    return reference_tuples(tuples(a), tuples(b), max_vals)


def out_words(ref, max_vals):
    """the reference as the primitive's 2 * (1 + 3 * max_vals) output words"""
    words = []
    for n_bad, lst in (ref[0:2], ref[2:4]):
        words.append(n_bad)
        for k in range(max_vals):
            words += list(lst[k] if k < len(lst) else PAD)
    return np.array(words, dtype=np.uint64)


# ---------------------------------------------------------------- cases
SIZES = (1, 2, 255, 256, 257, 1000, 4097, 1 << 16)


def distinct_column(rng, n, dim, lo=0):
    """n distinct canonical values: component 0 runs over lo + a shuffled range
    (the other components random), so two calls with disjoint ranges share no value"""
    col = rng.integers(0, P, size=(dim, n), dtype=np.uint64)
    col[0] = (np.uint64(lo) + rng.permutation(n).astype(np.uint64)) * np.uint64(7919) + np.uint64(3)
    return col


class Case:
    def __init__(self, name, a, b, max_vals=16, same=False, expect=None):
        self.name, self.a, self.b, self.max_vals, self.same = name, a, b, max_vals, same
        self.expect = expect  # what the construction promises (the reference must agree)

    def reference(self):
        return reference(self.a, self.b, self.max_vals)


def cases(n, dim, seed=0):
    """the cases of one size and dimension (those that need a larger size are left out at small n)"""
    rng = np.random.default_rng([seed, n, dim])
    out = []
    a = distinct_column(rng, n, dim)
    out.append(Case("permuted_distinct", a, a[:, rng.permutation(n)], expect=(0, [], 0, [])))
    if n >= 3:
        k = n // 3
        rep = np.concatenate([a[:, :k]] * 3 + [a[:, k:n - 2 * k]], axis=1)[:, rng.permutation(n)]
        out.append(Case("permuted_repeats", rep, rep[:, rng.permutation(n)], expect=(0, [], 0, [])))
    out.append(Case("same_pointer", a, a, same=True, expect=(0, [], 0, [])))
    for tag, row in (("row0", 0), ("middle", n // 2), ("last", n - 1)):
        b = a.copy()
        b[0, row] = np.uint64(P - 2)  # a value no column holds (component 0 of the others is below 2^40)
        out.append(Case("one_changed_" + tag, a, b, expect=(1, [(row, 1, 0)], 1, [(row, 0, 1)])))
    if n >= 8:
        # one value 3 times in a against 2 times in b (a spare value takes its third row there), b shuffled
        a2 = a.copy()
        ra = sorted(rng.choice(n, 3, replace=False).tolist())
        for r in ra[1:]:
            a2[:, r] = a[:, ra[0]]
        b2 = a2.copy()
        b2[0, ra[2]] = np.uint64(P - 2)
        perm = rng.permutation(n)  # row j of b is row perm[j] of b2
        where = {int(r): j for j, r in enumerate(perm)}
        v_b, spare_b = min(where[ra[0]], where[ra[1]]), where[ra[2]]
        out.append(Case("three_against_two", a2, b2[:, perm],
                        expect=(1, [(ra[0], 3, 2)], 2, sorted([(v_b, 3, 2), (spare_b, 0, 1)]))))
    if n >= 2 and dim == 3:
        b = a.copy()
        b[2, n // 2] = (b[2, n // 2] + np.uint64(1)) % np.uint64(P)
        out.append(Case("last_component", a, b, expect=(1, [(n // 2, 1, 0)], 1, [(n // 2, 0, 1)])))
    # canonicalisation: v < 2^32 - 1 in a against v + p in b (v + p < 2^64)
    small = np.zeros((dim, n), np.uint64)
    small[:] = rng.permutation(min(n, 2**32 - 1)).astype(np.uint64)[None, :]
    for c in range(dim):
        small[c] = np.roll(small[c], c)
    out.append(Case("canonical", small, small + np.uint64(P), expect=(0, [], 0, [])))
    # more mismatches than max_vals: all 2n values distinct
    b = distinct_column(rng, n, dim, lo=n)
    for mv in (16, 4096):
        exp = (n, [(i, 1, 0) for i in range(min(n, mv))], n, [(i, 0, 1) for i in range(min(n, mv))])
        out.append(Case("all_distinct_%d" % mv, a, b, max_vals=mv, expect=exp))
    out.append(Case("counts_only", a, b, max_vals=0, expect=(n, [], n, [])))
    if n == 1 << 16:
        # the selector case: n - 1 copies of one value and one other in a, n copies in b
        sa = np.repeat(a[:, :1], n, axis=1)
        sb = sa.copy()
        sa[:, 40000] = a[:, 1]
        out.append(Case("selector", sa, sb, expect=(2, [(0, n - 1, n), (40000, 1, 0)], 1, [(0, n - 1, n)])))
    return out


# ---------------------------------------------------------------- the prover's diagnosis
def perm_reference(inst, cm1_rows, k=0, max_vals=16):
    """what z_diag() reports for permutation check k of a SyntheticStark trace (row-major cm1):
    the reference on the (A, B) against the (C, D) tuples -- f = A + u B + gamma and
    t = C + u D + gamma are injective in the tuple for all but a negligible share of (u, gamma)"""
    a, b, c, d = inst.perms[k]["cols"]
    rows = np.asarray(cm1_rows, dtype=np.uint64) % np.uint64(P)
    ta = [(int(x), int(y)) for x, y in zip(rows[:, a], rows[:, b])]
    tb = [(int(x), int(y)) for x, y in zip(rows[:, c], rows[:, d])]
    n_a, la, n_b, lb = reference_tuples(ta, tb, max_vals)
    return {"n_num": n_a, "num": la, "n_den": n_b, "den": lb}
