"""Circom .exec images (execFile.hpp:48-64) for zkgpu.Exec and
zkgpu.stark.Stark.set_exec: u64 words [nAdds, nSMap, adds[4 nAdds],
sMap[nSMap nCols]]; add i = (idx_1, idx_2, c, d) writes slot sizeWitness + i,
sMap[nCols i + j] is the slot of row i, column j (0: empty).

make_image packs the two tables; exec_from_rows factors a given trace into a
witness and an image whose hand-off gives the trace back (test inputs: the
real circuits' .exec files are not in the repository)."""
import numpy as np

P = 0xFFFFFFFF00000001


def make_image(adds, smap):
    """adds: (nAdds, 4) of (idx_1, idx_2, c, d); smap: (nSMap, nCols) slots -> the image's u64 words"""
    adds = np.asarray(adds, dtype=np.uint64).reshape(-1, 4)
    smap = np.asarray(smap, dtype=np.uint64)
    if smap.ndim != 2:
        raise ValueError("smap must be (nSMap, nCols)")
    head = np.array([adds.shape[0], smap.shape[0]], dtype=np.uint64)
    return np.concatenate([head, adds.reshape(-1), smap.reshape(-1)])


def split_image(image, n_cols):
    """-> (adds (nAdds, 4), smap (nSMap, n_cols)) views of an image"""
    image = np.asarray(image, dtype=np.uint64).reshape(-1)
    na, ns = int(image[0]), int(image[1])
    if image.size != 2 + 4 * na + ns * n_cols:
        raise ValueError("image of %d words, not 2 + 4 x %d + %d x %d" % (image.size, na, ns, n_cols))
    return image[2:2 + 4 * na].reshape(na, 4), image[2 + 4 * na:].reshape(ns, n_cols)


def exec_from_rows(rows, rng=None, add_share=0.125):
    """rows (N, nCols) uint64 -> (witness, image) with the hand-off of
    (witness, image) equal to rows mod p, cell for cell.

    Slot 0 holds the constant 1 (circom's), every distinct value of rows one
    further witness slot (some stored as value + p where that fits a u64).
    About add_share of the cells read an add's slot instead: the add takes
    two earlier slots (witness or add, slot 0 included) and a coefficient c
    from the edge values, and d = (value - tmp[idx_1] c) / tmp[idx_2] closes
    it.  Of the zero cells left, half use index 0 (empty), the others the
    witness slot that holds 0."""
    rng = rng if rng is not None else np.random.default_rng(0)
    rows = np.ascontiguousarray(rows, dtype=np.uint64) % np.uint64(P)
    n, n_cols = rows.shape
    vals, inv = np.unique(rows.reshape(-1), return_inverse=True)
    wit = np.concatenate([np.ones(1, np.uint64), vals])
    lift = (wit < np.uint64(2**32 - 1)) & (rng.random(wit.size) < 0.5)
    lift[0] = False
    wit[lift] += np.uint64(P)  # the same element, not canonical
    sw = wit.size
    smap = (inv.reshape(n, n_cols) + 1).astype(np.uint64)
    zero = rows == 0
    smap[zero & (rng.random(rows.shape) < 0.5)] = 0

    tmp = [int(v) % P for v in wit]
    nonzero = [k for k, v in enumerate(tmp) if v]
    edge = [0, 1, P - 1, P, P + 1, 2**64 - 1]
    cells = np.flatnonzero(rng.random(n * n_cols) < add_share)
    adds = np.zeros((cells.size, 4), np.uint64)
    flat = smap.reshape(-1)
    for i, cell in enumerate(cells):
        v = int(rows.reshape(-1)[cell])
        a = int(rng.integers(0, sw + i))
        b = nonzero[int(rng.integers(0, len(nonzero)))]
        c = edge[int(rng.integers(0, 6))] if rng.random() < 0.5 else int(rng.integers(0, 2**64, dtype=np.uint64))
        d = (v - tmp[a] * c) % P * pow(tmp[b], -1, P) % P
        adds[i, 0], adds[i, 1], adds[i, 2], adds[i, 3] = a, b, c, d
        tmp.append(v)
        if v:
            nonzero.append(sw + i)
        flat[cell] = sw + i
    return wit, make_image(adds, smap)
