"""The case module of the plookup hash tables (tests/h1h2_cases.py), on the CPU:
the two restatements of h12_hash agree, every collision case forms the probe
chain it promises, the C oracle agrees with the Python reference on every case
(the missing row included), and the sharded reference reassembles to it."""
import time

import numpy as np
import pytest

import h1h2_cases as hc

P = hc.P


# ---------------------------------------------------------------- the restated hash
def test_numpy_hash_is_the_integer_hash():
    rng = np.random.default_rng(1)
    for dim in (1, 3):
        keys = rng.integers(0, P, size=(dim, 500), dtype=np.uint64)
        edge = [[0] * dim, [P - 1] * dim, [1] * dim, [2**32 - 1] * dim, [2**32] * dim, [P - 1, 0, P - 1][:dim]]
        keys = np.concatenate([keys, np.array(edge, dtype=np.uint64).T], axis=1)
        h = hc.hash_np(keys)
        for j in range(keys.shape[1]):
            k = tuple(int(x) for x in keys[:, j])
            assert int(h[j]) == hc.hash_int(k), k
            for world in (1, 2, 3, 8, 2**32 - 1):
                o = hc.owner_int(int(h[j]), world)
                assert 0 <= o < world and int(hc.owner_np(h[j:j + 1], world)[0]) == o
    # a dim-3 hash chains over the components: it is not the dim-1 hash of any one of them
    assert hc.hash_int((5, 0, 0)) != hc.hash_int((5,)) and hc.hash_int((0, 0, 5)) != hc.hash_int((5, 0, 0))


def test_table_sizes():
    for n, m2, m4 in ((0, 1, 0), (1, 2, 4), (2, 4, 8), (3, 8, 16), (255, 512, 1024), (256, 512, 1024),
                      (257, 1024, 2048), (1000, 2048, 4096), (4096, 8192, 16384)):
        assert (hc.table_size_2n(n), hc.table_size_4n(n)) == (m2, m4)


def test_search_is_quick():
    """48 keys of one home slot, every size and both dims, both tables: well under a second in total"""
    rng = np.random.default_rng(2)
    t0 = time.perf_counter()
    for n in hc.SIZES:
        for dim in (1, 3):
            for size in hc.TABLES.values():
                mask = size(n) - 1
                keys = hc.homed(rng, dim, mask, mask // 2, 48)
                assert keys.shape == (dim, 48) and len(set(hc.tuples(keys))) == 48
                assert np.all(keys < np.uint64(P)) and np.all(hc.hash_np(keys) & np.uint64(mask) == mask // 2)
    spent = time.perf_counter() - t0
    print("48 homed keys x %d searches: %.3f s" % (len(hc.SIZES) * 4, spent))
    keys = hc.homed_owned(rng, 3, 511, 7, 2, 1, 48)
    assert np.all(hc.owner_np(hc.hash_np(keys), 2) == 1) and np.all(hc.hash_np(keys) & np.uint64(511) == 7)
    assert spent < 5.0  # (a loaded machine: the figure itself is printed above)


# ---------------------------------------------------------------- what the collision cases promise
def occupied(keys, mask):
    """the slots a linear-probe table of mask + 1 slots holds after the keys are inserted one by one:
    {slot: key}"""
    slots = {}
    for k in keys:
        h = hc.hash_int(k) & mask
        while h in slots:
            h = (h + 1) & mask
        slots[h] = k
    return slots


def run_length(slots, start, mask):
    """occupied slots from `start` on (cyclic) up to the first empty one"""
    k = 0
    while ((start + k) & mask) in slots and k <= mask:
        k += 1
    return k


def runs(slots, mask):
    """the maximal cyclic runs of occupied slots, as (first slot, length)"""
    out = []
    for s in slots:
        if ((s - 1) & mask) not in slots:
            out.append((s, run_length(slots, s, mask)))
    return out or ([(0, mask + 1)] if slots else [])


@pytest.mark.parametrize("dim", [1, 3])
@pytest.mark.parametrize("n", hc.SIZES)
def test_collision_cases_keep_their_promises(n, dim):
    """The occupied SET of a linear-probe table does not depend on the order of insertion (a key
    displaced by another takes the slot that one would have taken), so what is asserted here of a
    one-by-one simulation holds on the GPU whichever thread wins a slot: only WHICH key sits in
    which slot of a run differs.  The simulation runs in two orders to show it."""
    names = [c.name for c in hc.cases(n, dim)]
    for want in ("same_slot", "miss_behind_chain_row0", "range_table", "lazy_both"):
        assert names.count(want) == (2 if "_slot" in want or "miss" in want else 1), names
    if n >= 255:
        for want in ("wrap", "miss_after_wrap", "dense_run", "miss_behind_chain", "miss_behind_chain_last"):
            assert names.count(want) == 2, names
    for c in hc.cases(n, dim):
        if c.table is None:
            continue
        mask = c.mask
        assert mask + 1 == hc.TABLES[c.table](n) and c.f.shape == c.t.shape == (dim, n)
        keys = c.table_keys()
        slots = occupied(keys, mask)
        assert set(slots) == set(occupied(keys[::-1], mask)), c.name  # any order, one set
        homes = {hc.hash_int(k) & mask for k in keys}
        tkeys = set(hc.tuples(c.t))
        if c.kind in ("same_slot", "wrap", "miss"):
            # one home slot, one run of as many slots as there are keys
            assert homes == {c.home} and len(tkeys) == c.run == min(n, hc.CHAIN), c.name
            assert runs(slots, mask) == [(c.home, len(keys))], c.name
        if c.kind == "wrap" or c.name == "miss_after_wrap":
            assert c.home == mask - 3 and mask in slots and 0 in slots, c.name
        if c.name in ("same_slot", "miss_behind_chain"):
            assert c.home + c.run <= mask + 1, c.name  # this chain does not wrap
        if c.kind == "dense_run":
            assert len(keys) == c.run == 64 and runs(slots, mask) == [(c.home, 64)], c.name
            per_home = [sum(1 for k in keys if hc.hash_int(k) & mask == (c.home + j) & mask) for j in range(32)]
            assert per_home == [2] * 32, c.name
            # two keys per home: whatever the order, half of them at least sit behind another's chain
            assert sum(1 for s, k in slots.items() if hc.hash_int(k) & mask != s) >= 32, c.name
        if c.kind == "miss":
            absent = hc.tuples(c.absent)
            rows = [i for i, k in enumerate(hc.tuples(c.f)) if k not in tkeys]
            assert min(rows) == c.miss and {hc.tuples(c.f)[i] for i in rows} == set(absent), c.name
            table_only = occupied(sorted(tkeys), mask)  # the 2n table holds t alone
            for k in absent:
                h = hc.hash_int(k) & mask
                # its home lies inside the run, the first empty slot behind the whole chain
                assert h == c.home and h in table_only and run_length(table_only, h, mask) == c.run, c.name
        else:
            assert c.miss is None and set(hc.tuples(c.f)) <= tkeys, c.name
        if c.name.startswith("last_component"):
            cols = np.concatenate([c.f, c.t], axis=1)
            assert len(set(cols[0].tolist())) == 1 and len(set(cols[1].tolist())) == 1, c.name
        # the padding the GPU tests put behind the columns would change the answer if read
        assert tuple(c.f_pad.tolist()) not in tkeys and tuple(c.t_pad.tolist()) in set(hc.tuples(c.f)), c.name


@pytest.mark.parametrize("dim", [1, 3])
def test_lazy_cases_hold_lazy_words(dim):
    for n in hc.SIZES:
        by = {c.name: c for c in hc.cases(n, dim)}
        comps = (0,) if dim == 1 else (1, 2)
        for name, cols in (("lazy_f", "f"), ("lazy_t", "t"), ("lazy_both", "ft")):
            c = by[name]
            for which in "ft":
                lazy = [bool(np.any(getattr(c, which)[k] >= np.uint64(P))) for k in range(dim)]
                if n >= 16:  # (a random half of the words: at small n it may be none)
                    assert lazy == [which in cols and k in comps for k in range(dim)], (name, which)
        c = by["lazy_t"]
        if n >= 16:
            h1, h2 = c.reference()
            assert np.any(h1 >= np.uint64(P)) and np.any(h2 >= np.uint64(P))  # the raw word is carried


# ---------------------------------------------------------------- the references
def oracle_result(oracle, c):
    rows = (lambda col: np.ascontiguousarray(col.T) if c.dim == 3 else col[0].copy())
    try:
        h1, h2 = oracle.h1h2(rows(c.f), rows(c.t))
    except ValueError as e:
        return str(e)
    return (h1.T if c.dim == 3 else h1[None]), (h2.T if c.dim == 3 else h2[None])


def same_result(ref, got):
    if isinstance(ref, hc.Missing):
        return isinstance(got, str) and got == str(ref)
    return not isinstance(got, str) and np.array_equal(ref[0], got[0]) and np.array_equal(ref[1], got[1])


@pytest.mark.parametrize("dim", [1, 3])
@pytest.mark.parametrize("n", hc.SIZES)
def test_oracle_is_the_reference_on_every_case(oracle, n, dim):
    for c in hc.cases(n, dim):
        ref = c.reference()
        assert same_result(ref, oracle_result(oracle, c)), c.name
        assert (ref.row if isinstance(ref, hc.Missing) else None) == c.miss, c.name


def test_reference_by_hand():
    """counts on the LAST row of a value, raw words out, the smallest missing row"""
    t = np.array([3, 5, 5 + P, 9], np.uint64)
    h1, h2 = hc.reference(np.array([5, 5, 9, 3 + P], np.uint64), t)
    assert [int(x) for x in h1[0]] == [3, 5, 5 + P, 9] and [int(x) for x in h2[0]] == [3, 5 + P, 5 + P, 9]
    with pytest.raises(hc.Missing, match="Number not included: w=1") as e:
        hc.reference(np.array([5, 7, 9, 8], np.uint64), t)
    assert e.value.row == 1
    h1, h2 = hc.reference_rows(np.array([[1, 2, 3]] * 2, np.uint64), np.array([[1, 2, 3], [1, 2, 3]], np.uint64))
    assert h1.shape == (2, 3) and np.array_equal(h1, h2)
    e0 = np.zeros((3, 0), np.uint64)
    assert hc.reference(e0, e0)[0].shape == (3, 0)


@pytest.mark.parametrize("dim", [1, 3])
@pytest.mark.parametrize("world", hc.WORLDS)
@pytest.mark.parametrize("n", hc.SHARD_SIZES)
def test_sharded_reference_reassembles(oracle, n, world, dim):
    cs = hc.sharded_cases(n, dim, world)
    names = [c.name for c in cs]
    assert names == [x for x in ("one_owner", "few_keys", "local_same_slot", "owner_same_slot", "repeat_across_ranks",
                                 "miss_not_first_rank")
                     if (world >= 2 or x not in ("few_keys", "miss_not_first_rank"))
                     and (world == 2 or x != "owner_same_slot")]
    nb = n // world
    for c in cs:
        ref = c.reference()
        assert same_result(ref, oracle_result(oracle, c)), c.name
        R = hc.sharded_reference(c.f, c.t, world)
        kt, kf = hc.tuples(c.t), hc.tuples(c.f)
        for s in range(world):
            # a sender's records: its distinct keys, each with the owner the hash names
            assert sum(R.n_t[s]) == len(set(kt[s * nb:(s + 1) * nb])), c.name
            assert sum(R.n_f[s]) == len(set(kf[s * nb:(s + 1) * nb])), c.name
            for o in range(world):
                for rec in R.t_recs[s][o] + R.f_recs[s][o]:
                    assert hc.owner_int(hc.hash_int(rec[:dim]), world) == o and rec[dim:3] == (0,) * (3 - dim)
                    assert s * nb <= rec[3] < (s + 1) * nb
        if isinstance(ref, hc.Missing):
            assert R.missing == ref.row == c.miss, c.name
        else:
            assert R.missing is None and sum(R.total) == 2 * n, c.name
            ms = np.concatenate(R.seg, axis=1)
            assert np.array_equal(ms[:, 0::2], ref[0]) and np.array_equal(ms[:, 1::2], ref[1]), c.name
            assert sum(R.ret.values()) == n, c.name  # every f row is counted once
        # what the case promises
        if c.name == "one_owner":
            assert [r > 0 for r in R.nrec] == [o == c.note["owner"] for o in range(world)]
        if c.name == "few_keys":
            assert len(set(kt)) == world - 1
        if c.name == "local_same_slot":
            mask, home = c.note["mask"], c.note["home"]
            assert mask + 1 == hc.table_size_2n(nb)
            for s in range(world):
                mine = set(kt[s * nb:(s + 1) * nb])
                assert len(mine) == min(nb, hc.CHAIN) and {hc.hash_int(k) & mask for k in mine} == {home}
                assert runs(occupied(sorted(mine), mask), mask) == [(home, len(mine))]
            assert len(set(kt)) == world * min(nb, hc.CHAIN)
        if c.name == "owner_same_slot":
            o, mask = c.note["owner"], c.note["mask"]
            assert R.nrec[o] == c.note["nrec"] and R.nrec[1 - o] == 0 and mask + 1 == hc.table_size_2n(R.nrec[o])
            keys = sorted(set(kt))
            assert runs(occupied(keys, mask), mask) == [(c.note["home"], len(keys))] and len(keys) == min(nb, 48)
        if c.name == "repeat_across_ranks":
            rows = c.note["rows"]
            k = kt[rows[0]]
            assert [i for i in range(n) if kt[i] == k] == sorted(set(rows))
            got = {r: R.ret[hc.key3(k) + (r,)] for r in rows[1:]}  # one record per rank: its largest row
            assert got[rows[-1]] == kf.count(k) > n // 5 and all(v == 0 for r, v in got.items() if r != rows[-1])
        if c.name == "miss_not_first_rank":
            assert c.miss >= nb and {o: m for o, m in enumerate(R.miss) if m is not None} == c.note["owner_miss"]
