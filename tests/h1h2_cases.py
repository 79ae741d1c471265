"""Plookup h1/h2 on adversarial hash tables: the restated hash of
csrc/h1h2.hip, the pure-Python references (whole columns and row-sharded) and
the case table of zkgpu_h1h2_dev, zkgpu_h1h2_shard_* and, at their table size,
zkgpu_multiset_diff_dev / zkgpu_lookup_misses_dev (include/zkgpu.h).

A column is a (dim, n) uint64 array (dim 1 or 3, component c of row i at
[c, i]), as the device holds it; a key is the canonical dim-tuple, so v and
v + p are one key.  The five tables of h1h2.hip are open-addressing tables
with linear probing over h12_hash: the builders below search keys by their
home slot (and owner), so that the cases form the probe chains, the wrap past
the last slot and the clusters that uniformly random keys never do.  No GPU."""
import functools
from collections import Counter

import numpy as np

P = 0xFFFFFFFF00000001
M64 = (1 << 64) - 1
T_VAL = M64  # a t record's val (h1h2.hip:220 H12S_T)
ABSENT = P - 2  # every component of a value no generated table holds


# ---------------------------------------------------------------- restated from csrc/h1h2.hip
def hash_int(key):
    """h12_hash (h1h2.hip:49-61) of a tuple of canonical components, plain integers"""
    h = 0x9E3779B97F4A7C15
    for k in key:
        z = (k + h) & M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        h = z ^ (z >> 31)
    return h


def hash_np(keys):
    """h12_hash (h1h2.hip:49-61) of the columns of a canonical (dim, k) uint64 array -> (k,) uint64"""
    keys = np.asarray(keys, dtype=np.uint64)
    h = np.full(keys.shape[1], 0x9E3779B97F4A7C15, np.uint64)
    for c in range(keys.shape[0]):
        z = keys[c] + h  # uint64 arrays wrap
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        h = z ^ (z >> np.uint64(31))
    return h


def owner_int(h, world):
    """h12s_owner (h1h2.hip:223-226): the rank that owns a key, from the hash's high half"""
    return ((h >> 32) * world) >> 32


def owner_np(h, world):
    return ((np.asarray(h, np.uint64) >> np.uint64(32)) * np.uint64(world)) >> np.uint64(32)


def table_size_2n(n):
    """2^k >= 2n slots: the table of t rows (h1h2_hash, h1h2.hip:141-142), a rank's local t and f
    tables from its nrows and an owner's table from its nrec (h12s_table_size, h1h2.hip:415-420)"""
    m = 1
    while m < 2 * n:
        m <<= 1
    return m


def table_size_4n(n):
    """2^k >= 4n slots: the multiset table of two columns (ms_table_size, h1h2.hip:584-590)"""
    if not n:
        return 0
    m = 1
    while m < 4 * n:
        m <<= 1
    return m


TABLES = {"2n": table_size_2n, "4n": table_size_4n}


# ---------------------------------------------------------------- the reference
class Missing(ValueError):
    """the reference's "Number not included" (polinomial.hpp:395-399); row = the smallest such f row"""

    def __init__(self, row):
        ValueError.__init__(self, "Number not included: w=%d" % row)
        self.row = row


def columns(col):
    col = np.asarray(col, dtype=np.uint64)
    return col.reshape(1, -1) if col.ndim == 1 else col


def tuples(col):
    """the canonical keys of a column's rows, as tuples of integers"""
    canon = columns(col) % np.uint64(P)
    return list(zip(*(canon[c].tolist() for c in range(canon.shape[0]))))


def counts(kf, kt):
    """the reference's counter after its two first loops (polinomial.hpp:349-401): every table row 1,
    plus the f rows with its key on the LAST table row with that key (the chain entry keeps the
    latest index, :380-383); raises Missing at the first f row without one"""
    last = {}
    for i, k in enumerate(kt):
        last[k] = i
    counter = [1] * len(kt)
    for i, k in enumerate(kf):
        j = last.get(k)
        if j is None:
            raise Missing(i)
        counter[j] += 1
    return counter


def reference(f, t):
    """polinomial.hpp:349-463 step by step on (dim, n) columns -> (h1, h2), the table's raw words"""
    f, t = columns(f), columns(t)
    n = t.shape[1]
    counter = counts(tuples(f), tuples(t))
    src1, src2 = np.zeros(n, np.int64), np.zeros(n, np.int64)
    idx = 0
    for i in range(n):  # the deal (:403-462)
        if counter[idx] == 0:
            idx += 1
        counter[idx] -= 1
        src1[i] = idx
        if counter[idx] == 0:
            idx += 1
        counter[idx] -= 1
        src2[i] = idx
    return t[:, src1], t[:, src2]


def reference_rows(f, t):
    """reference() on the oracle's layout: f, t are (n,) or (n, dim), and so are h1, h2"""
    f, t = np.asarray(f, dtype=np.uint64), np.asarray(t, dtype=np.uint64)
    if t.ndim == 1:
        h1, h2 = reference(f, t)
        return h1[0], h2[0]
    h1, h2 = reference(f.T, t.T)
    return np.ascontiguousarray(h1.T), np.ascontiguousarray(h2.T)


def key3(k):
    return tuple(k) + (0,) * (3 - len(k))


class Sharded:
    """calculateH1H2 over `world` ranks of nb = n / world rows, step by step (include/zkgpu.h
    zkgpu_h1h2_shard_*):
      t_recs[s][o], f_recs[s][o]  the records sender s routes to owner o, sorted 5-tuples
                                  (k0, k1, k2, global row, val): a distinct t key with its largest
                                  row and val ~0, a distinct f key with its smallest row and its count
      n_t[s][o], n_f[s][o]        their numbers; nrec[o] what owner o receives
      ret[(k0, k1, k2, row)]      the owner's return for a t record: the key's f count over all ranks
                                  if the row is the key's largest, else 0
      miss[o], missing            the smallest f row whose key has no t row: per owner, over all
      cnt[s], start[s], total[s]  the sender's counts (1 + return), their exclusive scan, their sum
      seg[s]                      the sender's segment of the multiset, (dim, total[s]) raw words"""


def sharded_reference(f, t, world):
    f, t = columns(f), columns(t)
    dim, n = t.shape
    assert world >= 1 and n % world == 0 and n >= world
    nb = n // world
    kf, kt = tuples(f), tuples(t)
    R = Sharded()
    R.world, R.nb = world, nb
    R.t_recs = [[[] for _ in range(world)] for _ in range(world)]
    R.f_recs = [[[] for _ in range(world)] for _ in range(world)]
    owner = {}
    for k in set(kf) | set(kt):
        owner[k] = owner_int(hash_int(k), world)
    t_last, f_count = {}, Counter(kf)  # over all ranks
    for i, k in enumerate(kt):
        t_last[k] = i
    for s in range(world):
        last, first, cnt = {}, {}, Counter()
        for i in range(s * nb, (s + 1) * nb):
            last[kt[i]] = i
            first.setdefault(kf[i], i)
            cnt[kf[i]] += 1
        for k, i in last.items():
            R.t_recs[s][owner[k]].append(key3(k) + (i, T_VAL))
        for k, i in first.items():
            R.f_recs[s][owner[k]].append(key3(k) + (i, cnt[k]))
        for o in range(world):
            R.t_recs[s][o].sort()
            R.f_recs[s][o].sort()
    R.n_t = [[len(R.t_recs[s][o]) for o in range(world)] for s in range(world)]
    R.n_f = [[len(R.f_recs[s][o]) for o in range(world)] for s in range(world)]
    R.nrec = [sum(R.n_t[s][o] + R.n_f[s][o] for s in range(world)) for o in range(world)]
    R.ret, R.miss = {}, [None] * world
    for s in range(world):
        for o in range(world):
            for rec in R.t_recs[s][o]:
                k = rec[:dim]
                R.ret[rec[:4]] = f_count.get(k, 0) if t_last[k] == rec[3] else 0
            for rec in R.f_recs[s][o]:
                if rec[:dim] not in t_last and (R.miss[o] is None or rec[3] < R.miss[o]):
                    R.miss[o] = rec[3]
    found = [m for m in R.miss if m is not None]
    R.missing = min(found) if found else None
    R.cnt, R.start, R.total, R.seg = [], [], [], []
    for s in range(world):
        cnt = np.ones(nb, np.int64)
        for o in range(world):
            for rec in R.t_recs[s][o]:
                cnt[rec[3] - s * nb] += R.ret[rec[:4]]
        start = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64)
        R.cnt.append(cnt)
        R.start.append(start)
        R.total.append(int(cnt.sum()))
        R.seg.append(np.repeat(t[:, s * nb:(s + 1) * nb], cnt, axis=1))
    return R


# ---------------------------------------------------------------- key builders by search
def search(rng, dim, count, keep, fixed=(), rate=1.0):
    """`count` distinct canonical keys (dim, count) whose hashes keep() selects: random keys,
    filtered (fixed = leading components every key shares; rate = the share keep() lets through)"""
    batch = int(min(1 << 20, max(1 << 12, 2 * count / rate)))
    found, seen = [], set()
    while len(found) < count:
        k = rng.integers(0, P, size=(dim, batch), dtype=np.uint64)
        for c, v in enumerate(fixed):
            k[c] = np.uint64(v)
        sel = k[:, keep(hash_np(k))]
        for j in range(sel.shape[1]):
            key = tuple(sel[:, j].tolist())
            if key not in seen and len(found) < count:
                seen.add(key)
                found.append(key)
    return np.array(found, dtype=np.uint64).T.reshape(dim, count)


def homed(rng, dim, mask, slot, count, fixed=()):
    """distinct canonical keys whose hash & mask == slot"""
    return search(rng, dim, count, lambda h: (h & np.uint64(mask)) == np.uint64(slot), fixed, 1.0 / (mask + 1))


def owned(rng, dim, world, owner, count):
    """distinct canonical keys that rank `owner` of `world` owns"""
    return search(rng, dim, count, lambda h: owner_np(h, world) == np.uint64(owner), (), 1.0 / world)


def homed_owned(rng, dim, mask, slot, world, owner, count):
    """distinct canonical keys with hash & mask == slot that rank `owner` of `world` owns"""
    return search(rng, dim, count,
                  lambda h: ((h & np.uint64(mask)) == np.uint64(slot)) & (owner_np(h, world) == np.uint64(owner)),
                  (), 1.0 / ((mask + 1) * world))


def homed_run(rng, dim, mask, slot0, nslots, per_slot):
    """per_slot distinct keys homed on each of the nslots slots from slot0 (mod mask + 1), slot by slot"""
    got = [[] for _ in range(nslots)]
    batch = int(min(1 << 20, max(1 << 12, 8 * per_slot * (mask + 1))))
    while any(len(g) < per_slot for g in got):
        k = rng.integers(0, P, size=(dim, batch), dtype=np.uint64)
        d = ((hash_np(k) & np.uint64(mask)) - np.uint64(slot0)) & np.uint64(mask)
        idx = np.nonzero(d < np.uint64(nslots))[0]
        for j in idx.tolist():
            g = got[int(d[j])]
            key = tuple(k[:, j].tolist())
            if len(g) < per_slot and key not in g:
                g.append(key)
    return np.array([key for g in got for key in g], dtype=np.uint64).T.reshape(dim, nslots * per_slot)


def distinct_column(rng, n, dim):
    """n distinct canonical values (component 0 a shuffled arithmetic progression, the others random)"""
    col = rng.integers(0, P, size=(dim, n), dtype=np.uint64)
    col[0] = rng.permutation(n).astype(np.uint64) * np.uint64(7919) + np.uint64(1 << 40)
    return col


# ---------------------------------------------------------------- cases
SIZES = (1, 2, 3, 255, 256, 257, 1000, 4096)
SHARD_SIZES = (48, 3072)
WORLDS = (1, 2, 3, 8)
CHAIN = 48  # keys of one home slot
RUN_SLOTS, RUN_PER_SLOT = 32, 2  # dense_run


class Case:
    """f, t: (dim, n) raw words.  table: the table the case aims at ("2n" / "4n", None: no table in
    particular) with its mask.  kind / home / run: what the construction promises of the occupied
    slots (tests/test_h1h2_cases.py checks it by simulation).  miss: the f row the reference must
    name, None when every f value is in t.  absent: the (dim, k) keys of f that t does not hold."""

    def __init__(self, name, f, t, table=None, kind=None, home=None, run=None, miss=None, absent=None, note=None):
        self.name, self.f, self.t = name, np.ascontiguousarray(f), np.ascontiguousarray(t)
        self.dim, self.n = self.t.shape
        self.table, self.kind, self.home, self.run, self.miss, self.absent = table, kind, home, run, miss, absent
        self.note = note or {}
        self.mask = TABLES[table](self.n) - 1 if table else None
        self._ref = None

    def reference(self):
        """(h1, h2), or the Missing the reference raises (computed once, never changed)"""
        if self._ref is None:
            try:
                self._ref = reference(self.f, self.t)
            except Missing as e:
                self._ref = e
        return self._ref

    def table_keys(self):
        """the distinct keys the aimed table ends up holding: those of t (2n), of f and t (4n)"""
        keys = tuples(self.t) + (tuples(self.f) if self.table == "4n" else [])
        return sorted(set(keys))

    @property
    def f_pad(self):
        """rows [n, ld) of f: a value no table holds (read, it would be a miss)"""
        return np.full(self.dim, ABSENT, np.uint64)

    @property
    def t_pad(self):
        """rows [n, ld) of t: the value most rows of f hold (read, it would take their counts)"""
        k = Counter(tuples(self.f)).most_common(1)[0][0]
        return np.array(k, dtype=np.uint64)


def spread(rng, keys, n):
    """t: a random draw of the keys with every key present; f: a random draw of t's rows"""
    k = keys.shape[1]
    idx = np.concatenate([np.arange(k), rng.integers(0, k, size=n - k)])
    t = keys[:, rng.permutation(idx)]
    return t[:, rng.integers(0, n, size=n)], t


def with_values(col, rows, vals):
    out = col.copy()
    for r, v in zip(rows, vals.T):
        out[:, r] = v
    return out


def collision_cases(rng, n, dim, table):
    """the cases that aim at one table size (those a size cannot hold are left out)"""
    m = TABLES[table](n)
    mask = m - 1
    K = min(n, CHAIN)
    out = []

    def chain_cases(tag, miss_tag, home, fixed=()):
        keys = homed(rng, dim, mask, home, K + 2, fixed)
        chain, absent = keys[:, :K], keys[:, K:]
        f, t = spread(rng, chain, n)
        out.append(Case(tag, f, t, table, kind=tag, home=home, run=K))
        # two absent keys of the same home: the probe has to walk the whole chain before it may say so
        if n >= 2:
            rows = (n // 3, (2 * n) // 3)
            out.append(Case(miss_tag, with_values(f, rows[::-1], absent), t, table, kind="miss", home=home, run=K,
                            miss=rows[0], absent=absent))
        return f, t, absent

    home = int(rng.integers(0, m - K + 1))  # the chain ends at or before the last slot
    f, t, absent = chain_cases("same_slot", "miss_behind_chain", home)
    rows = (0, n - 1) if n >= 2 else (0,)
    out.append(Case("miss_behind_chain_row0", with_values(f, rows, absent), t, table, kind="miss", home=home, run=K,
                    miss=0, absent=absent[:, :len(rows)]))
    if n >= 2:
        out.append(Case("miss_behind_chain_last", with_values(f, (n - 1,), absent[:, 1:]), t, table, kind="miss",
                        home=home, run=K, miss=n - 1, absent=absent[:, 1:]))
    if K >= 5:
        # three before the last slot: the chain runs over slot mask into slot 0
        chain_cases("wrap", "miss_after_wrap", mask - 3)
    if n >= RUN_SLOTS * RUN_PER_SLOT:
        slot0 = int(rng.integers(0, m))  # (a run may itself wrap)
        keys = homed_run(rng, dim, mask, slot0, RUN_SLOTS, RUN_PER_SLOT)
        f, t = spread(rng, keys, n)
        out.append(Case("dense_run", f, t, table, kind="dense_run", home=slot0, run=RUN_SLOTS * RUN_PER_SLOT))
    if dim == 3:
        # keys that agree in components 0 and 1: only the last one tells them apart
        fixed = tuple(int(x) for x in rng.integers(0, P, size=2, dtype=np.uint64))
        home = int(rng.integers(0, m - K + 1))
        keys = homed(rng, dim, mask, home, K + 1, fixed)
        f, t = spread(rng, keys[:, :K], n)
        out.append(Case("last_component", f, t, table, kind="same_slot", home=home, run=K))
        out.append(Case("last_component_miss", with_values(f, (n // 2,), keys[:, K:]), t, table, kind="miss",
                        home=home, run=K, miss=n // 2, absent=keys[:, K:]))
    return out


def small_column(base, dim):
    """(n,) small integers -> a (dim, n) column whose rows are equal exactly where base is"""
    base = np.asarray(base, dtype=np.uint64)
    if dim == 1:
        return base.reshape(1, -1).copy()
    return np.stack([base, base ^ np.uint64(0x5555), base * np.uint64(3) + np.uint64(1)])


def lazify(rng, col):
    """v -> v + p (the same element, v + p < 2^64) on a random half of the words below 2^32 - 1:
    component 0 of a dim-1 column, components 1 and 2 of a dim-3 column"""
    out = col.copy()
    for c in ((0,) if col.shape[0] == 1 else (1, 2)):
        pick = (rng.integers(0, 2, size=col.shape[1]) == 1) & (out[c] < np.uint64(2**32 - 1))
        out[c, pick] += np.uint64(P)
    return out


def plookup_cases(rng, n, dim):
    """tables shaped like a plookup's, and non-canonical words"""
    out = []
    draw = (lambda t: t[:, rng.integers(0, n, size=n)])
    t = small_column(np.arange(n), dim)
    out.append(Case("range_table", draw(t), t))
    t = small_column(np.arange(n) % 256, dim)  # heavy repeats: the last row of a value takes its counts
    out.append(Case("byte_table", draw(t), t))
    t = small_column(np.full(n, 5), dim)
    out.append(Case("one_value_table", t.copy(), t))
    # f all one value: one thread scatters n + 1 copies
    t = distinct_column(rng, n, dim)
    out.append(Case("f_one_value_row0", np.repeat(t[:, :1], n, axis=1), t))
    out.append(Case("f_one_value_last", np.repeat(t[:, n - 1:], n, axis=1), t))
    if n >= 2:
        t2 = t.copy()
        t2[:, n // 2] = t2[:, 0]  # rows 0 and n / 2 hold one value: row n / 2 takes the counts
        out.append(Case("f_one_value_repeat", np.repeat(t2[:, :1], n, axis=1), t2))
    # lazy words: keys compare canonically, h1 / h2 carry the table's raw word
    base = distinct_column(rng, n // 2 + 1, dim)
    for c in ((0,) if dim == 1 else (1, 2)):
        base[c] = np.roll(rng.permutation(n // 2 + 1).astype(np.uint64), c)
    f, t = spread(rng, base, n)
    out.append(Case("lazy_f", lazify(rng, f), t))
    out.append(Case("lazy_t", f, lazify(rng, t)))
    out.append(Case("lazy_both", lazify(rng, f), lazify(rng, t)))
    return out


@functools.lru_cache(maxsize=None)
def cases(n, dim, seed=0):
    """the whole-column cases of one size and dimension"""
    rng = np.random.default_rng([seed, n, dim])
    return collision_cases(rng, n, dim, "2n") + collision_cases(rng, n, dim, "4n") + plookup_cases(rng, n, dim)


@functools.lru_cache(maxsize=None)
def sharded_cases(n, dim, world, seed=0):
    """the cases of the row-sharded steps: `world` ranks of nb = n / world rows each"""
    rng = np.random.default_rng([seed, n, dim, world])
    nb = n // world
    out = []
    draw = (lambda t: t[:, rng.integers(0, n, size=n)])
    # every key owned by the LAST rank: the others receive nothing (nrec = 0)
    t = owned(rng, dim, world, world - 1, n)
    out.append(Case("one_owner", draw(t), t, note={"owner": world - 1}))
    if world >= 2:
        f, t = spread(rng, rng.integers(0, P, size=(dim, world - 1), dtype=np.uint64), n)
        out.append(Case("few_keys", f, t))
    # every rank's rows of t hold keys of ONE home slot of its local table (sized from nrows); the
    # ranks' key sets are disjoint, so a rank's f rows hold up to min(nb, world * K) of them
    m = table_size_2n(nb)
    K = min(nb, CHAIN)
    home = int(rng.integers(0, m))
    keys = homed(rng, dim, m - 1, home, world * K)
    t = np.concatenate([spread(rng, keys[:, r * K:(r + 1) * K], nb)[1] for r in range(world)], axis=1)
    out.append(Case("local_same_slot", draw(t), t, note={"mask": m - 1, "home": home}))
    if world == 2:
        # K keys of one owner AND one home slot of that owner's table: every rank holds every key in
        # t and in f, so the owner receives 2 K records from each rank, 4 K in all
        m = table_size_2n(4 * K)
        home = int(rng.integers(0, m))
        keys = homed_owned(rng, dim, m - 1, home, world, 1, K)
        t = np.concatenate([spread(rng, keys, nb)[1] for r in range(world)], axis=1)
        f = np.concatenate([spread(rng, keys, nb)[1] for r in range(world)], axis=1)
        out.append(Case("owner_same_slot", f, t, note={"owner": 1, "nrec": 4 * K, "mask": m - 1, "home": home}))
    # one table value on every rank: the largest global row takes all counts
    t = distinct_column(rng, n, dim)
    for r in range(world):
        t[:, r * nb + nb // 2] = t[:, 0]
    f = draw(t)
    f[:, 1::5] = t[:, :1]
    out.append(Case("repeat_across_ranks", f, t, note={"rows": [0] + [r * nb + nb // 2 for r in range(world)]}))
    if world >= 2:
        # two absent values, of the last and of the first owner; the smaller row is the last owner's
        # and lies on rank 1
        t = distinct_column(rng, n, dim)
        a, b = owned(rng, dim, world, world - 1, 1), owned(rng, dim, world, 0, 1)
        f = with_values(draw(t), (nb + 1, n - 1, nb + 2), np.concatenate([a, a, b], axis=1))
        out.append(Case("miss_not_first_rank", f, t, miss=nb + 1, absent=np.concatenate([a, b], axis=1),
                        note={"owner_miss": {world - 1: nb + 1, 0: nb + 2}}))
    return out
