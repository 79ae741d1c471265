"""CPU side of the lookup-miss listing: the pure-Python reference of
tests/lookup_cases.py against a brute-force double loop on tiny inputs and
against what each case's construction promises, and the workspace formula of
zkgpu_lookup_misses_dev (host only)."""
import numpy as np
import pytest

import lookup_cases as lc

P = lc.P


def test_reference_small_by_hand():
    f = np.array([5, 9, 5, 11, 9, 7], np.uint64)
    t = np.array([7, 5, 5, 3, 3, 3], np.uint64)
    # 9 misses on rows 1 and 4, 11 on row 3
    assert lc.reference(f, t, 16) == (3, 2, [(1, 2), (3, 1)])
    assert lc.reference(f, t, 1) == (3, 2, [(1, 2)])
    assert lc.reference(f, t, 0) == (3, 2, [])
    assert lc.reference(f + np.uint64(P), t, 16) == (3, 2, [(1, 2), (3, 1)])  # v + p is v
    assert lc.reference(t, t, 16) == (0, 0, [])
    assert list(lc.out_words((3, 2, [(1, 2), (3, 1)]), 3)) == [3, 2, 1, 2, 3, 1, 2**64 - 1, 0]


@pytest.mark.parametrize("dim", [1, 3])
def test_reference_against_brute_force(dim):
    rng = np.random.default_rng(dim)
    for n in (1, 2, 3, 7, 20):
        for _ in range(20):
            # few distinct values: hits, misses and repeats of both all occur
            f = rng.integers(0, 4, size=(dim, n), dtype=np.uint64)
            t = rng.integers(0, 3, size=(dim, n), dtype=np.uint64)
            lift = rng.integers(0, 2, size=(dim, n), dtype=np.uint64) * np.uint64(P)
            for mv in (0, 2, 16):
                assert lc.reference(f + lift, t, mv) == lc.brute_force(f, t, mv)
                assert lc.reference(f, t + lift, mv) == lc.brute_force(f, t, mv)
    for n in (1, 2, 40):
        for case in lc.cases(n, dim):
            assert case.reference() == lc.brute_force(case.f, case.t, case.max_vals), case.name


@pytest.mark.parametrize("dim", [1, 3])
@pytest.mark.parametrize("n", lc.SIZES)
def test_reference_on_case_table(n, dim):
    names = set()
    for case in lc.cases(n, dim):
        names.add(case.name)
        assert case.expect is not None, case.name
        n_rows, n_vals, lst = case.expect
        assert case.reference() == (n_rows, n_vals, lst[:case.max_vals]), case.name
        assert case.f.shape == case.t.shape == (dim, n)
        assert lc.out_words(case.reference(), case.max_vals).size == 2 + 2 * case.max_vals
    if n == 0:
        assert names == {"empty_0", "empty_16"}
        return
    assert {"no_miss", "same_pointer", "miss_row0", "miss_last", "all_rows_one_value", "all_rows_distinct_0",
            "all_rows_distinct_16", "all_rows_distinct_4096", "canonical_f", "canonical_t"} <= names
    assert ("straddle_256" in names) == (n > 257) and ("straddle_1024" in names) == (n > 1025)
    assert ("twenty_values" in names) == (n >= 210)
    assert ("last_component" in names) == (dim == 3)


def test_workspace_bytes_formula():
    import zkgpu
    f = zkgpu.lookup_misses_workspace_bytes
    for n in [0, 1, 2, 3, 255, 256, 257, 1000, 1024, 1025, 4097, 1 << 16, (1 << 16) + 1, 1 << 23, 1 << 28]:
        m = 1
        while m < 4 * n:
            m <<= 1
        if n == 0:
            m = 0
        blocks = (n + 1023) // 1024
        assert f(n) == 16 * m + 8 * n + 8 * ((blocks + 1) // 2) + 8 * 4097 + 8, n
        assert f(n) <= zkgpu.multiset_diff_workspace_bytes(n), n  # one allocation serves both
