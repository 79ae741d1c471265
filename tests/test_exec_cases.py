"""The .exec hand-off's reference model (tests/exec_cases.py) against a
hand-computed example, the shapes of the shared cases, and
zkgpu.exec_file.exec_from_rows through the model.  CPU only."""
import numpy as np

import exec_cases as xc

P = xc.P


def test_model_on_a_hand_computed_example():
    # slots 0..2 the witness (2^64 - 1 = 2^32 - 2 mod p), slots 3..5 the adds
    witness = np.array([1, 2, 3 + P], dtype=np.uint64)
    adds = [(1, 2, 5, 7),              # 2 * 5 + 3 * 7 = 31
            (3, 0, 2, P - 1),          # 31 * 2 - 1 = 61
            (4, 4, P - 1, 2**64 - 1)]  # -61 + 61 (2^32 - 2) = 61 (2^32 - 3)
    smap = [[3, 4, 5], [0, 1, 2]]
    image = np.array([3, 2] + [x for a in adds for x in a] + [x for r in smap for x in r], dtype=np.uint64)
    got = xc.model(witness, image, 3, 3)
    assert got.tolist() == [[31, 61, 261993004873], [0, 2, 3], [0, 0, 0]]
    assert xc.schedule(image, 3) == ([1, 2, 3], 3, 1)


def test_cases_have_the_shapes_they_are_named_for():
    by = {c["name"]: c for c in xc.cases()}
    sched = {k: xc.schedule(c["image"], c["size_witness"]) for k, c in by.items()}
    assert sched["b_chain_5000"][1:] == (5000, 1)
    assert sched["c_grid_tail_grid"][1:] == (302, 3)
    lev_d = np.bincount(sched["d_levels_T-1_T_T+1"][0])[1:]
    assert lev_d.tolist() == [xc.T - 1, xc.T, xc.T + 1] and sched["d_levels_T-1_T_T+1"][2] == 2
    assert sched["e_no_adds"][1:] == (0, 0)
    assert {c["n_cols"] for c in by.values()} == {1, 12, 18}
    for c in by.values():
        w = xc.witness_of(c, 1)
        assert w[0] == 1 and w[1] == 0 and w[2] == P
    assert set(xc.EDGE) <= set(int(x) for x in xc.witness_of(by["a_random_dag"], 1))
    assert set(xc.EDGE) <= set(int(x) for x in by["a_random_dag"]["image"][2:2 + 4 * 2000].reshape(-1, 4)[:, 2:].ravel())


def test_exec_from_rows_round_trips_through_the_model():
    from zkgpu import exec_file
    rng = np.random.default_rng(5)
    rows = rng.integers(0, P, size=(64, 7), dtype=np.uint64)
    rows[rng.random(rows.shape) < 0.3] = 0
    rows[3] = rows[9]  # repeated values share a slot
    rows[5, 2] = P - 1
    witness, image = exec_file.exec_from_rows(rows, np.random.default_rng(6))
    assert witness[0] == 1 and witness.size <= 1 + np.unique(rows).size
    adds, smap = exec_file.split_image(image, 7)
    assert adds.shape[0] > 20 and smap.shape == (64, 7)
    assert (smap[rows == 0] == 0).any() and (smap[rows == 0] != 0).any()
    assert np.array_equal(xc.model(witness, image, 7, 64), rows)
    # non-canonical rows come back reduced
    rows2 = rows.copy()
    rows2[0, 0] = P + 5
    w2, im2 = exec_file.exec_from_rows(rows2, np.random.default_rng(7))
    assert np.array_equal(xc.model(w2, im2, 7, 64), rows2 % np.uint64(P))
    assert np.array_equal(exec_file.make_image(adds, smap), image)
