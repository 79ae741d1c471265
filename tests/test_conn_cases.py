"""CPU side of the connection breaks: the pure-Python reference of
tests/conn_cases.py by hand and against what each case's construction
promises, the property that keeps it honest (the grand product closes exactly
when the reference finds nothing), and the host-only calls of
zkgpu_conn_breaks_dev through libzkgpu.so: the workspace formula and the
refusal of colliding coset shifts."""
import functools

import numpy as np
import pytest

import conn_cases as cc

P = cc.P


@functools.lru_cache(maxsize=None)
def table(n_bits, k):
    return cc.cases(n_bits, k)


def test_reference_small_by_hand():
    # n = 4, k = 2: cells 0..3 are column 0, 4..7 column 1; 1 <-> 6 swapped, the rest fixed points
    ks, ids = cc.default_ks(2), cc.identities(cc.default_ks(2), 2)
    assert ids[0] == 1 and ids[4] == 12 and ids[1] == cc.omega(2) and pow(ids[1], 4, P) == 1
    perm = [0, 6, 2, 3, 4, 5, 1, 7]
    s = np.array([ids[t] for t in perm], np.uint64).reshape(2, 4)
    a = np.array([10, 5, 12, 13, 14, 15, 5, 17], np.uint64).reshape(2, 4)
    assert cc.reference(a, s, ks, 2, 16) == ((0, 0, 0), [], [])
    a[1, 2] = 6  # cell 6: both links of the 2-cycle break, both naming it
    want = [(1, 6, 5, 6), (6, 1, 6, 5)]
    assert cc.reference(a, s, ks, 2, 16) == ((2, 0, 0), want, [])
    assert cc.reference(a, s, ks, 2, 1) == ((2, 0, 0), want[:1], [])
    assert cc.reference(a + np.uint64(P), s, ks, 2, 16) == ((2, 0, 0), want, [])  # v + p is v
    a[0, 0] = 99  # a fixed point never breaks
    assert cc.reference(a, s, ks, 2, 16)[0] == (2, 0, 0)
    s[0, 3] = 0  # cell 3 foreign: nobody names cell 3 any more
    assert cc.reference(a, s, ks, 2, 16) == ((2, 1, 1), want, [(3, 0)])
    s[0, 3] = ids[2]  # two cells name cell 2
    assert cc.reference(a, s, ks, 2, 16) == ((3, 0, 1), [(1, 6, 5, 6), (3, 2, 13, 12), (6, 1, 6, 5)], [])
    words = cc.out_words(((2, 1, 1), want, [(3, 0)]), 3)
    none = 2**64 - 1
    assert list(words) == [2, 1, 1, 1, 6, 5, 6, 6, 1, 6, 5, none, 0, 0, 0, 3, 0, none, 0, none, 0]


@pytest.mark.parametrize("n_bits,k", cc.SHAPES)
def test_reference_on_case_table(n_bits, k):
    names = set()
    for case in table(n_bits, k):
        names.add(case.name)
        counts, breaks, foreign = case.reference()
        if case.expect is not None:
            assert counts == case.expect, case.name
        assert len(breaks) == min(counts[0], case.max_vals) and len(foreign) == min(counts[1], case.max_vals)
        assert breaks == sorted(breaks) and foreign == sorted(foreign), case.name
        assert case.a.shape == case.s.shape == (k, 1 << n_bits)
        assert cc.out_words(case.reference(), case.max_vals).size == 3 + 6 * case.max_vals
        if case.name.startswith("one_off") or case.name == "own_ks_one_off":
            off = {"one_off_first": 0, "one_off_middle": (k << n_bits) // 2}.get(case.name, (k << n_bits) - 1)
            assert [b[0] == off or b[1] == off for b in breaks] == [True, True], case.name  # both name it
    cells = k << n_bits
    always = {"clean_random", "identity", "one_cycle", "fixed_point_off", "canonical", "own_ks_clean",
              "foreign_zero_at_0", "foreign_coset_at_0", "foreign_zero_plus_p_at_0",
              "foreign_zero_at_%d" % (cells - 1), "foreign_coset_at_%d" % (cells - 1)}
    assert always <= names
    larger = {"one_off_first", "one_off_last", "one_off_middle", "all_broken_0", "all_broken_1", "all_broken_16",
              "duplicate_target", "duplicate_target_broken", "own_ks_one_off", "own_ks_mismatch"}
    assert (larger <= names) == (cells >= 2) and (cells >= 2 or not (larger & names))
    if cells > 16:
        assert [c.expect[0] for c in table(n_bits, k) if c.name == "all_broken_16"] == [cells]  # past the list


@pytest.mark.parametrize("n_bits,k", cc.SHAPES)
def test_product_closes_exactly_when_clean(n_bits, k):
    rng = np.random.default_rng([7, n_bits, k])
    for case in table(n_bits, k):
        beta, gamma = (int(x) for x in rng.integers(1, P, size=2, dtype=np.uint64))
        clean = case.reference()[0] == (0, 0, 0)
        assert cc.closes(case.a, case.s, case.ks, n_bits, beta, gamma) == clean, case.name


def test_ks_collision_reference():
    assert cc.ks_collision(cc.default_ks(12), 22) is None
    assert cc.ks_collision([1, 0], 3) == "conn_breaks: ks[1] is zero"
    assert cc.ks_collision([3, 5, 3 * cc.omega(3) % P], 3) == "conn_breaks: the cosets of ks[0] and ks[2] collide"
    assert cc.ks_collision([3, 5, 3 * cc.omega(4) % P], 3) is None  # w_16 is outside the subgroup of order 8


def test_workspace_bytes_formula():
    import zkgpu
    f = zkgpu.conn_breaks_workspace_bytes
    last = 0
    for n_bits, k in [(0, 1), (0, 3), (1, 1), (3, 1), (5, 2), (5, 3), (6, 12), (8, 3), (10, 2), (10, 3), (16, 5),
                      (22, 12), (23, 2), (25, 64), (28, 8)]:
        c = k << n_bits
        blocks = (c + 1023) // 1024
        assert f(1 << n_bits, k) == 16 * c + 8 * ((c + 1) // 2) + 8 * ((blocks + 1) // 2) + 16 * 4097 + 8, (n_bits, k)
    for c in sorted(k << b for b in range(0, 20, 3) for k in (1, 2, 3, 12, 64)):  # monotone in the cells
        now = max(f(n, k) for n, k in ((c, 1), (1, c)))
        assert f(c, 1) == f(1, c) and now >= last
        last = now


def test_colliding_ks_are_refused_without_a_gpu():
    import zkgpu
    w3 = cc.omega(3)
    for ks, k, n_bits in (([3, 5, 3 * w3 % P], 3, 3), ([1, 0], 2, 3), ([7, 7 + P], 2, 0), ([1, 12, 144, 1], 4, 10)):
        with pytest.raises(zkgpu.ZkgpuError) as e:
            zkgpu.conn_ks_check(ks, k, n_bits)
        assert str(e.value) == "zkgpu_conn_ks_check failed (-2): " + cc.ks_collision(ks, n_bits)
    zkgpu.conn_ks_check(None, 64, 28)  # the default shifts never collide
    zkgpu.conn_ks_check([3, 5, 3 * cc.omega(4) % P], 3, 3)
    # the primitive itself judges its arguments before it looks for a GPU
    dummy = np.zeros(8, np.uint64)
    with pytest.raises(zkgpu.ZkgpuError) as e:
        zkgpu.conn_breaks_dev(dummy, dummy, 8, None, dummy, 8, None, 3, [3, 5, 3 * w3 % P], 3, 0)
    assert str(e.value) == "zkgpu_conn_breaks_dev failed (-2): conn_breaks: the cosets of ks[0] and ks[2] collide"
