"""The circom .exec hand-off (zkgpu_exec_*, include/zkgpu.h) restated over
Python ints, and the cases the CPU and GPU tests share.

model() is the reference's loop, Circom*::getCommitedPols
(main.recursive1.cpp:343-394): tmp = the witness, then one slot per add, then
the sMap gather with index 0 as "empty" and zero rows past nSMap.

Every case draws its witness words and coefficients from {0, 1, p - 1, p,
p + 1, 2^64 - 1, random u64}."""
import numpy as np

P = 0xFFFFFFFF00000001
EDGE = [0, 1, P - 1, P, P + 1, 2**64 - 1]
T = 1024  # the widest level a single-workgroup launch takes (csrc/exec_plan.hpp EXEC_TAIL_MAX)


def model(witness, image, n_cols, n):
    """-> (n, n_cols) uint64, canonical: main.recursive1.cpp:343-394"""
    image = [int(x) for x in np.asarray(image).reshape(-1)]
    n_adds, n_smap = image[0], image[1]
    assert len(image) == 2 + 4 * n_adds + n_smap * n_cols and n >= n_smap
    tmp = [int(x) % P for x in np.asarray(witness).reshape(-1)]
    for i in range(n_adds):
        a, b, c, d = image[2 + 4 * i:6 + 4 * i]
        assert a < len(tmp) and b < len(tmp)
        tmp.append((tmp[a] * c + tmp[b] * d) % P)
    smap = image[2 + 4 * n_adds:]
    out = np.zeros((n, n_cols), np.uint64)
    for i in range(n_smap):
        for j in range(n_cols):
            s = smap[n_cols * i + j]
            out[i, j] = tmp[s] if s else 0
    return out


def schedule(image, size_witness, tail=T):
    """-> (levels per add, n_levels, n_segments): the level of an add is 1 + its
    operands' highest (witness slots 0); a level wider than `tail` is a segment,
    a run of consecutive narrower levels one segment"""
    image = np.asarray(image).reshape(-1)
    n_adds = int(image[0])
    lev = []
    for i in range(n_adds):
        a, b = int(image[2 + 4 * i]), int(image[3 + 4 * i])
        lev.append(1 + max(lev[a - size_witness] if a >= size_witness else 0,
                           lev[b - size_witness] if b >= size_witness else 0))
    n_levels = max(lev, default=0)
    width = np.bincount(np.asarray(lev, dtype=np.int64), minlength=n_levels + 1)[1:]
    segs, in_tail = 0, False
    for w in width:
        if w > tail:
            segs, in_tail = segs + 1, False
        elif not in_tail:
            segs, in_tail = segs + 1, True
    return lev, n_levels, segs


def words(rng, k):
    """k u64 words, half of them edge values"""
    w = rng.integers(0, 2**64, size=k, dtype=np.uint64)
    pick = rng.random(k) < 0.5
    w[pick] = np.array(EDGE, dtype=np.uint64)[rng.integers(0, len(EDGE), size=int(pick.sum()))]
    return w


def witness_of(case, seed):
    """a witness of the case: slot 0 = 1, slot 1 = 0 and slot 2 = p (two zeros), edge values and random words"""
    rng = np.random.default_rng(seed)
    w = words(rng, case["size_witness"])
    w[0] = 1
    if w.size > 2:
        w[1], w[2] = 0, P
    return w


def _image(adds, smap):
    adds = np.asarray(adds, dtype=np.uint64).reshape(-1, 4)
    head = np.array([adds.shape[0], smap.shape[0]], dtype=np.uint64)
    return np.concatenate([head, adds.reshape(-1), smap.reshape(-1).astype(np.uint64)])


def _smap(rng, n_smap, n_cols, n_slots):
    """random slots, one cell in ten empty (index 0); with rows enough, column 0 starts with the two
    zero-valued witness slots and an empty cell"""
    s = rng.integers(0, n_slots, size=(n_smap, n_cols), dtype=np.uint64)
    s[rng.random(s.shape) < 0.1] = 0
    if n_smap >= 3 and n_slots > 2:
        s[0, 0], s[1, 0], s[2, 0] = 1, 2, 0
    return s


def _adds(rng, a, b):
    a = np.asarray(a, dtype=np.uint64)
    return np.stack([a, np.asarray(b, dtype=np.uint64), words(rng, a.size), words(rng, a.size)], axis=1)


def _case(name, sw, n_cols, adds, n_smap, n, ld, rng):
    adds = np.asarray(adds, dtype=np.uint64).reshape(-1, 4)
    smap = _smap(rng, n_smap, n_cols, sw + adds.shape[0])
    return {"name": name, "size_witness": sw, "n_cols": n_cols, "image": _image(adds, smap), "n": n, "ld": ld}


def cases():
    rng = np.random.default_rng(20240)
    out = []
    # (a) a random DAG: operands anywhere earlier, tmp[0] among them
    sw, na = 300, 2000
    a = [int(rng.integers(0, sw + i)) for i in range(na)]
    b = [int(rng.integers(0, sw + i)) for i in range(na)]
    a[0], b[1] = 0, 0
    out.append(_case("a_random_dag", sw, 12, _adds(rng, a, b), 1000, 1000, 1000, rng))
    # (b) a pure chain of depth 5000: the single-workgroup tail; nSMap < n < ld, one column
    sw, na = 40, 5000
    a = [int(rng.integers(0, sw))] + [sw + i - 1 for i in range(1, na)]
    b = [int(rng.integers(0, sw)) for _ in range(na)]
    out.append(_case("b_chain_5000", sw, 1, _adds(rng, a, b), 700, 1000, 1100, rng))
    # (c) a level of 70000 independent adds, a chain, a wide level again: grid, tail, grid
    sw, wide, chain = 500, 70000, 300
    a = list(rng.integers(0, sw, size=wide))
    b = list(rng.integers(0, sw, size=wide))
    for k in range(chain):
        a.append(sw + wide + k - 1 if k else sw + int(rng.integers(0, wide)))
        b.append(int(rng.integers(0, sw + wide)))
    last = sw + wide + chain - 1
    a += [last] * wide
    b += list(rng.integers(0, sw + wide, size=wide))
    out.append(_case("c_grid_tail_grid", sw, 18, _adds(rng, a, b), 1000, 1000, 1000, rng))
    # (d) consecutive levels of exactly T - 1, T and T + 1 adds
    sw = 64
    a = list(rng.integers(0, sw, size=T - 1)) + list(sw + rng.integers(0, T - 1, size=T)) + \
        list(sw + T - 1 + rng.integers(0, T, size=T + 1))
    b = list(rng.integers(0, sw, size=3 * T))
    out.append(_case("d_levels_T-1_T_T+1", sw, 12, _adds(rng, a, b), 1000, 1000, 1000, rng))
    # (e) no adds: the gather alone
    out.append(_case("e_no_adds", 200, 12, np.zeros((0, 4), np.uint64), 1000, 1000, 1024, rng))
    # (f) further sMap shapes: 18 columns with nSMap < n < ld, one column with nSMap = n
    sw, na = 100, 50
    a = [int(rng.integers(0, sw + i)) for i in range(na)]
    b = [int(rng.integers(0, sw + i)) for i in range(na)]
    out.append(_case("f_18_cols_short_smap", sw, 18, _adds(rng, a, b), 999, 1000, 1001, rng))
    out.append(_case("f_1_col_full_smap", sw, 1, _adds(rng, a, b), 1000, 1000, 1000, rng))
    # nSMap = 0: every cell is zero
    out.append(_case("f_no_smap", sw, 12, _adds(rng, a, b), 0, 1000, 1000, rng))
    return out
