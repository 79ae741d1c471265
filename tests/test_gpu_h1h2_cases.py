"""The hash tables of csrc/h1h2.hip on the cases of tests/h1h2_cases.py: long
probe chains, chains that wrap past the last slot, clusters, misses behind a
chain, plookup-shaped tables and lazy words.  zkgpu_h1h2_dev against the
Python reference; the sharded steps (zkgpu_h1h2_shard_*) one by one against the
sharded reference; zkgpu_multiset_diff_dev / zkgpu_lookup_misses_dev on the
collision cases built for their table size.  Bit-exact: raw words, no
tolerance.  The columns sit in images of four different leading dimensions
whose rows [n, ld) would change the answer if read, the outputs start as a
sentinel word with guard words behind them, and every call runs twice: the two
results must be equal (nothing may depend on which thread wins a slot) and
every padding and guard word intact."""
import ctypes

import numpy as np
import pytest

import h1h2_cases as hc
import lookup_cases as lc
import multiset_cases as mc

pytestmark = pytest.mark.gpu

SENT = np.uint64(0xA5C3A5C3F00DFACE)
SENT32 = 0x5A5AC3C3
GUARD = 8
NONE = (1 << 64) - 1


def lds(n):
    """h1, h2, f, t: four different leading dimensions above n"""
    return n + 3, n + 5, n + 8, n + 13


def image(col, ld, pad):
    """the column at leading dimension ld: rows [n, ld) hold pad, guard words follow"""
    dim, n = col.shape
    img = np.full(dim * ld + GUARD, SENT, np.uint64)
    v = img[:dim * ld].reshape(dim, ld)
    v[:, :n] = col
    v[:, n:] = np.asarray(pad, np.uint64).reshape(dim, 1)
    return img


def blank(words):
    return np.full(words + GUARD, SENT, np.uint64)


def split(img, dim, ld, n):
    """an output image -> (its n rows, everything else: padding rows and guard)"""
    body = img[:dim * ld].reshape(dim, ld)
    return body[:, :n].copy(), np.concatenate([body[:, n:].ravel(), img[dim * ld:]])


def all_sent(words):
    return bool(np.all(words == SENT))


# ---------------------------------------------------------------- zkgpu_h1h2_dev
def run_h1h2(zkgpu, case):
    """-> (rc, missing_row, error text, h1 rows, h2 rows); padding, guards and inputs checked"""
    dim, n = case.dim, case.n
    ld1, ld2, fld, tld = lds(n)
    f_img, t_img = image(case.f, fld, case.f_pad), image(case.t, tld, case.t_pad)
    d_f, d_t = zkgpu.to_device(f_img), zkgpu.to_device(t_img)
    d_h1, d_h2 = zkgpu.to_device(blank(dim * ld1)), zkgpu.to_device(blank(dim * ld2))
    miss = ctypes.c_uint64(12345)
    rc = zkgpu.lib().zkgpu_h1h2_dev(d_h1.data_ptr(), ld1, d_h2.data_ptr(), ld2, d_f.data_ptr(), fld, d_t.data_ptr(),
                                    tld, n, dim, ctypes.byref(miss))
    text = zkgpu.lib().zkgpu_last_error().decode() if rc else ""
    zkgpu.synchronize()
    h1, rest1 = split(zkgpu.from_device(d_h1), dim, ld1, n)
    h2, rest2 = split(zkgpu.from_device(d_h2), dim, ld2, n)
    assert all_sent(rest1) and all_sent(rest2), (case.name, "h1 / h2 written outside their n rows")
    assert np.array_equal(zkgpu.from_device(d_f), f_img) and np.array_equal(zkgpu.from_device(d_t), t_img), case.name
    return rc, miss.value, text, h1, h2


def check_h1h2(zkgpu, case):
    first, again = run_h1h2(zkgpu, case), run_h1h2(zkgpu, case)
    tag = (case.name, case.table)
    assert first[:3] == again[:3] and np.array_equal(first[3], again[3]) and np.array_equal(first[4], again[4]), \
        (tag, "two runs differ")
    rc, miss, text, h1, h2 = first
    ref = case.reference()
    if isinstance(ref, hc.Missing):
        assert ref.row == case.miss
        assert (rc, miss) == (-2, ref.row), (tag, rc, miss, ref.row)
        assert text == "calculateH1H2: Number not included: w=%d" % ref.row, (tag, text)
    else:
        assert (rc, miss, text) == (0, NONE, ""), (tag, rc, miss, text)
        bad = np.nonzero(np.any(h1 != ref[0], axis=0) | np.any(h2 != ref[1], axis=0))[0]
        assert bad.size == 0, (tag, "first wrong row", int(bad[0]), h1[:, bad[0]], ref[0][:, bad[0]], h2[:, bad[0]],
                               ref[1][:, bad[0]])


@pytest.mark.parametrize("dim", [1, 3])
@pytest.mark.parametrize("n", hc.SIZES)
def test_h1h2_vs_reference(zkgpu, n, dim):
    for case in hc.cases(n, dim):
        check_h1h2(zkgpu, case)


def test_h1h2_python_wrapper_names_the_row(zkgpu):
    case = [c for c in hc.cases(1000, 3) if c.name == "miss_after_wrap" and c.table == "2n"][0]
    n = case.n
    d_f, d_t = zkgpu.to_device(case.f), zkgpu.to_device(case.t)
    d_h = zkgpu.to_device(blank(6 * n))
    assert zkgpu.h1h2_dev(d_h, n, d_h.data_ptr() + 24 * n, n, d_f, n, d_t, n, n, 3) == case.miss == n // 3


def test_h1h2_no_rows(zkgpu):
    """n = 0 returns 0 and writes nothing"""
    d_in = zkgpu.to_device(blank(64))
    for dim in (1, 3):
        d_h1, d_h2 = zkgpu.to_device(blank(64)), zkgpu.to_device(blank(64))
        miss = ctypes.c_uint64(12345)
        rc = zkgpu.lib().zkgpu_h1h2_dev(d_h1.data_ptr(), 8, d_h2.data_ptr(), 8, d_in.data_ptr(), 8, d_in.data_ptr(),
                                        8, 0, dim, ctypes.byref(miss))
        zkgpu.synchronize()
        assert (rc, miss.value) == (0, NONE)
        assert all_sent(zkgpu.from_device(d_h1)) and all_sent(zkgpu.from_device(d_h2))


def test_h1h2_refusals(zkgpu):
    d_in = zkgpu.to_device(np.zeros(1024, np.uint64))
    d_h1, d_h2 = zkgpu.to_device(blank(1024)), zkgpu.to_device(blank(1024))
    big = 1 << 31
    for args, message in (((d_h1, 100, d_h2, 100, d_in, 100, d_in, 100, 100, 2), "h1h2: dim must be 1 or 3"),
                          ((d_h1, 100, d_h2, 100, d_in, 100, d_in, 100, 100, 0), "h1h2: dim must be 1 or 3"),
                          ((d_h1, big, d_h2, big, d_in, big, d_in, big, big, 1), "h1h2: n too large"),
                          ((d_h1, big, d_h2, big, d_in, big, d_in, big, big, 3), "h1h2: n too large"),
                          ((d_h1, 99, d_h2, 100, d_in, 100, d_in, 100, 100, 3), "h1h2: ld < n"),
                          ((d_h1, 100, d_h2, 99, d_in, 100, d_in, 100, 100, 3), "h1h2: ld < n"),
                          ((d_h1, 100, d_h2, 100, d_in, 99, d_in, 100, 100, 3), "h1h2: ld < n"),
                          ((d_h1, 100, d_h2, 100, d_in, 100, d_in, 99, 100, 3), "h1h2: ld < n")):
        with pytest.raises(zkgpu.ZkgpuError) as e:
            zkgpu.h1h2_dev(*args)
        assert str(e.value) == "zkgpu_h1h2_dev failed (-2): " + message
    zkgpu.synchronize()
    assert all_sent(zkgpu.from_device(d_h1)) and all_sent(zkgpu.from_device(d_h2))  # nothing was queued


# ---------------------------------------------------------------- the sharded steps
def cuts(a, b):
    """the multiset piece [a, b) cut again: a first piece of length 1, then a cut at an odd position"""
    pts = {a, b}
    if b - a >= 2:
        pts.add(a + 1)
    odd = ((a + b) // 2) | 1
    if a < odd < b:
        pts.add(odd)
    pts = sorted(pts)
    return list(zip(pts[:-1], pts[1:]))


def run_sharded(zkgpu, case, W, R):
    """calculateH1H2 through zkgpu_h1h2_shard_* for W ranks of n / W rows, the exchanges of
    host/sharded_starks.hpp h1h2_sharded emulated on the host; every step against the sharded
    reference R.  Returns what must not change from run to run."""
    import torch
    dim, n = case.dim, case.n
    nb = n // W
    ld1, ld2, fld, tld = lds(n)
    f_img, t_img = image(case.f, fld, case.f_pad), image(case.t, tld, case.t_pad)
    d_f, d_t = zkgpu.to_device(f_img), zkgpu.to_device(t_img)
    tag = (case.name, W)
    seen = {"records": [], "ret": []}
    # ---- route: every rank's records, bucketed by owner, t records first
    d_recs, words, n_t, n_f = [], [], [], []
    for r in range(W):
        cap = 2 * nb
        d_rec = zkgpu.to_device(blank(5 * cap))
        nt, nf = zkgpu.h1h2_shard_route(d_rec, cap, d_f.data_ptr() + 8 * r * nb, fld, d_t.data_ptr() + 8 * r * nb, tld,
                                        nb, r * nb, dim, W)
        zkgpu.synchronize()
        nt, nf = [int(x) for x in nt], [int(x) for x in nf]
        assert (nt, nf) == (R.n_t[r], R.n_f[r]), (tag, "route: bucket sizes of rank", r)
        w = zkgpu.from_device(d_rec)
        tot = sum(nt) + sum(nf)
        assert all_sent(w[5 * tot:]), (tag, "route wrote past its records")
        rows = w[:5 * tot].reshape(tot, 5)
        at = 0
        for o in range(W):
            for k, want in ((nt[o], R.t_recs[r][o]), (nf[o], R.f_recs[r][o])):
                got = sorted(tuple(x) for x in rows[at:at + k].tolist())
                assert got == want, (tag, "route: records of rank", r, "for owner", o)
                seen["records"].append(got)
                at += k
        if r == 0:  # one record short: refused, nothing written
            d_short = zkgpu.to_device(blank(5 * cap))
            with pytest.raises(zkgpu.ZkgpuError, match="%d records exceed the %d-record buffer" % (tot, tot - 1)):
                zkgpu.h1h2_shard_route(d_short, tot - 1, d_f.data_ptr(), fld, d_t.data_ptr(), tld, nb, 0, dim, W)
            zkgpu.synchronize()
            assert all_sent(zkgpu.from_device(d_short)), (tag, "a refused route wrote records")
        d_recs.append(d_rec)
        words.append(rows)
        n_t.append(nt)
        n_f.append(nf)
    nr = (lambda s, o: n_t[s][o] + n_f[s][o])
    soff = [np.concatenate([[0], np.cumsum([nr(s, o) for o in range(W)])]).astype(np.int64) for s in range(W)]
    # ---- owner: the buckets every rank sent it, concatenated
    rets, roffs, misses = [], [], []
    for o in range(W):
        roff = np.concatenate([[0], np.cumsum([nr(s, o) for s in range(W)])]).astype(np.int64)
        nrec = int(roff[-1])
        assert nrec == R.nrec[o]
        recv = blank(5 * nrec)
        for s in range(W):
            recv[5 * roff[s]:5 * roff[s + 1]] = words[s][soff[s][o]:soff[s][o + 1]].ravel()
        d_recv, d_ret = zkgpu.to_device(recv), zkgpu.to_device(blank(nrec))
        miss = zkgpu.h1h2_shard_owner(d_ret, d_recv, nrec, dim)
        zkgpu.synchronize()
        assert miss == R.miss[o], (tag, "owner", o, "missing row", miss, R.miss[o])
        ret = zkgpu.from_device(d_ret)
        assert all_sent(ret[nrec:]), (tag, "owner wrote past its records")
        assert np.array_equal(zkgpu.from_device(d_recv), recv)
        want = [R.ret[tuple(rec[:4])] if rec[4] == hc.T_VAL else 0 for rec in recv[:5 * nrec].reshape(nrec, 5).tolist()]
        assert ret[:nrec].tolist() == want, (tag, "owner", o, "returns")
        seen["ret"].append(sorted(zip((tuple(x) for x in recv[:5 * nrec].reshape(nrec, 5).tolist()), want)))
        rets.append(ret[:nrec])
        roffs.append(roff)
        misses.append(miss)
    found = [m for m in misses if m is not None]
    seen["missing"] = min(found) if found else None
    assert seen["missing"] == R.missing, tag
    if found:
        return seen
    # ---- counts: each t record's return back at its sender
    tots, d_starts, d_cnts = [], [], []
    for s in range(W):
        ret_in = blank(2 * nb)
        for o in range(W):
            k = n_t[s][o]  # (the returns of the f records are not sent back)
            ret_in[soff[s][o]:soff[s][o] + k] = rets[o][roffs[o][s]:roffs[o][s] + k]
        d_start = torch.full((nb + GUARD,), SENT32, dtype=torch.int32, device="cuda:0")
        d_cnt = torch.full((nb + GUARD,), SENT32, dtype=torch.int32, device="cuda:0")
        tot = zkgpu.h1h2_shard_counts(d_start, d_cnt, d_recs[s], zkgpu.to_device(ret_in), int(soff[s][-1]), nb, s * nb)
        zkgpu.synchronize()
        start, cnt = d_start.cpu().numpy(), d_cnt.cpu().numpy()
        assert np.all(start[nb:] == SENT32) and np.all(cnt[nb:] == SENT32), (tag, "counts wrote past nrows")
        assert np.array_equal(cnt[:nb], R.cnt[s]) and np.array_equal(start[:nb], R.start[s]), (tag, "counts of rank", s)
        assert tot == R.total[s], (tag, "total of rank", s)
        tots.append(tot)
        d_starts.append(d_start)
        d_cnts.append(d_cnt)
    assert sum(tots) == 2 * n
    off = np.concatenate([[0], np.cumsum(tots)]).astype(np.int64)
    # ---- deal, then every piece to the rank that holds its rows
    d_h1, d_h2 = zkgpu.to_device(blank(dim * ld1)), zkgpu.to_device(blank(dim * ld2))
    pieces = {"one": 0, "odd": 0, "last_row": 0}
    for s in range(W):
        tot = tots[s]
        seg_ld = tot + 7
        d_seg = zkgpu.to_device(blank(dim * seg_ld))
        zkgpu.h1h2_shard_deal(d_seg, seg_ld, d_t.data_ptr() + 8 * s * nb, tld, d_starts[s], d_cnts[s], nb, dim)
        zkgpu.synchronize()
        seg, rest = split(zkgpu.from_device(d_seg), dim, seg_ld, tot)
        assert all_sent(rest), (tag, "deal wrote past the segment")
        assert np.array_equal(seg, R.seg[s]), (tag, "segment of rank", s)
        for e in range(W):
            a, b = max(int(off[s]), 2 * e * nb), min(int(off[s]) + tot, 2 * (e + 1) * nb)
            if a >= b:
                continue
            for x, y in cuts(a, b):
                pieces["one"] += y - x == 1
                pieces["odd"] += x % 2 == 1
                pieces["last_row"] += y == 2 * (e + 1) * nb
                zkgpu.h1h2_shard_place(d_h1.data_ptr() + 8 * e * nb, ld1, d_h2.data_ptr() + 8 * e * nb, ld2,
                                       d_seg.data_ptr() + 8 * (x - int(off[s])), seg_ld, x, y - x, e * nb, dim)
        zkgpu.synchronize()  # (the segment is released with the next one)
    assert pieces["one"] and pieces["odd"] and pieces["last_row"] >= W, (tag, pieces)
    h1, rest1 = split(zkgpu.from_device(d_h1), dim, ld1, n)
    h2, rest2 = split(zkgpu.from_device(d_h2), dim, ld2, n)
    assert all_sent(rest1) and all_sent(rest2), (tag, "place wrote outside the n rows")
    assert np.array_equal(zkgpu.from_device(d_f), f_img) and np.array_equal(zkgpu.from_device(d_t), t_img), tag
    ref = case.reference()
    assert np.array_equal(h1, ref[0]) and np.array_equal(h2, ref[1]), (tag, "h1 / h2")
    seen["h"] = (h1.tobytes(), h2.tobytes())
    return seen


@pytest.mark.parametrize("dim", [1, 3])
@pytest.mark.parametrize("world", hc.WORLDS)
@pytest.mark.parametrize("n", hc.SHARD_SIZES)
def test_sharded_steps(zkgpu, n, world, dim):
    for case in hc.sharded_cases(n, dim, world):
        R = hc.sharded_reference(case.f, case.t, world)
        first = run_sharded(zkgpu, case, world, R)
        again = run_sharded(zkgpu, case, world, R)
        assert first == again, (case.name, "two runs differ")
        assert first["missing"] == case.miss
        check_h1h2(zkgpu, case)  # and the whole columns on one rank


@pytest.mark.parametrize("dim", [1, 3])
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_steps_on_collision_cases(zkgpu, world, dim):
    """the whole-column chains (same_slot, wrap, dense_run, the misses) through the sharded steps: a
    rank's local tables and the owners' are smaller tables with other home slots, the result is the
    same; blocks of 255 rows"""
    n = 255 * world
    done = []
    for case in hc.collision_cases(np.random.default_rng([7, world, dim]), n, dim, "2n"):
        R = hc.sharded_reference(case.f, case.t, world)
        assert run_sharded(zkgpu, case, world, R)["missing"] == case.miss
        done.append(case.name)
    assert {"same_slot", "wrap", "dense_run", "miss_behind_chain", "miss_after_wrap"} <= set(done)


def test_sharded_owner_without_records(zkgpu):
    """nrec = 0: nothing to return, nothing missing, nothing written"""
    d_recv, d_ret = zkgpu.to_device(blank(5)), zkgpu.to_device(blank(1))
    for dim in (1, 3):
        assert zkgpu.h1h2_shard_owner(d_ret, d_recv, 0, dim) is None
    zkgpu.synchronize()
    assert all_sent(zkgpu.from_device(d_ret))


def test_sharded_refusals(zkgpu):
    import torch
    d_in = zkgpu.to_device(np.zeros(1024, np.uint64))
    d_out, d_out2 = zkgpu.to_device(blank(2048)), zkgpu.to_device(blank(2048))
    d_i32 = torch.full((256,), SENT32, dtype=torch.int32, device="cuda:0")
    top = (1 << 32) - 100  # row0 + nrows = 2^32
    sh = "h1h2 (sharded): "
    calls = (
        ("route", (d_out, 200, d_in, 100, d_in, 100, 100, 0, 1, 0), sh + "empty world or block"),
        ("route", (d_out, 200, d_in, 100, d_in, 100, 0, 0, 1, 2), sh + "empty world or block"),
        ("route", (d_out, 200, d_in, 99, d_in, 100, 100, 0, 3, 2), sh + "ld < nrows"),
        ("route", (d_out, 200, d_in, 100, d_in, 99, 100, 0, 1, 2), sh + "ld < nrows"),
        ("route", (d_out, 200, d_in, 100, d_in, 100, 100, top, 1, 2), sh + "rows beyond 2^32"),
        ("route", (d_out, 200, d_in, 100, d_in, 100, 100, 0, 2, 2), sh + "dim must be 1 or 3"),
        ("route", (d_out, 200, d_in, 1 << 31, d_in, 1 << 31, 1 << 31, 0, 1, 2), sh + "n too large"),
        ("owner", (d_out, d_in, 100, 2), sh + "dim must be 1 or 3"),
        ("owner", (d_out, d_in, 1 << 31, 1), sh + "n too large"),
        ("counts", (d_i32, d_i32, d_in, d_in, 0, 0, 0), sh + "empty block"),
        ("counts", (d_i32, d_i32, d_in, d_in, 0, 1 << 31, 0), sh + "n too large"),
        ("deal", (d_out, 100, d_in, 100, d_i32, d_i32, 100, 2), sh + "dim must be 1 or 3"),
        ("place", (d_out, 100, d_out2, 100, d_in, 100, 2 * 50 - 1, 10, 50, 1), sh + "position before the block"),
        ("place", (d_out, 100, d_out2, 100, d_in, 100, 0, 10, 1, 3), sh + "position before the block"),
        ("place", (d_out, 100, d_out2, 100, d_in, 100, 100, 10, 50, 2), sh + "dim must be 1 or 3"),
    )
    for step, args, message in calls:
        with pytest.raises(zkgpu.ZkgpuError) as e:
            getattr(zkgpu, "h1h2_shard_" + step)(*args)
        assert str(e.value) == "zkgpu_h1h2_shard_%s failed (-2): %s" % (step, message), (step, args[1:])
    # an empty piece and an empty block are no error and write nothing
    zkgpu.h1h2_shard_place(d_out, 100, d_out2, 100, d_in, 100, 0, 0, 50, 1)
    zkgpu.h1h2_shard_deal(d_out, 100, d_in, 100, d_i32, d_i32, 0, 3)
    zkgpu.synchronize()
    assert all_sent(zkgpu.from_device(d_out)) and all_sent(zkgpu.from_device(d_out2))  # nothing was queued
    assert bool(torch.all(d_i32 == SENT32))


# ---------------------------------------------------------------- the 4n table: multiset difference, lookup misses
KINDS_4N = ("same_slot", "wrap", "dense_run", "miss_behind_chain", "miss_behind_chain_row0", "miss_behind_chain_last",
            "miss_after_wrap", "last_component", "last_component_miss")
MAX_VALS = 64  # above the 48 + 2 keys of a chain: every value is listed


def cases_4n(n, dim):
    return [c for c in hc.cases(n, dim) if c.table == "4n" and c.name in KINDS_4N]


def run_multiset(zkgpu, case):
    dim, n = case.dim, case.n
    _, _, a_ld, b_ld = lds(n)
    a_img, b_img = image(case.f, a_ld, case.f_pad), image(case.t, b_ld, case.t_pad)
    d_a, d_b = zkgpu.to_device(a_img), zkgpu.to_device(b_img)
    words = 2 * (1 + 3 * MAX_VALS)
    d_out = zkgpu.to_device(blank(words))
    zkgpu.multiset_diff_dev(d_out, d_a, a_ld, d_b, b_ld, n, dim, MAX_VALS)
    zkgpu.synchronize()
    got = zkgpu.from_device(d_out)
    assert all_sent(got[words:]), case.name
    assert np.array_equal(zkgpu.from_device(d_a), a_img) and np.array_equal(zkgpu.from_device(d_b), b_img), case.name
    return got[:words]


def run_lookup(zkgpu, case):
    dim, n = case.dim, case.n
    _, _, f_ld, t_ld = lds(n)
    f_img, t_img = image(case.f, f_ld, case.f_pad), image(case.t, t_ld, case.t_pad)
    d_f, d_t = zkgpu.to_device(f_img), zkgpu.to_device(t_img)
    words = 2 + 2 * MAX_VALS
    d_out = zkgpu.to_device(blank(words))
    zkgpu.lookup_misses_dev(d_out, d_f, f_ld, d_t, t_ld, n, dim, MAX_VALS)
    zkgpu.synchronize()
    got = zkgpu.from_device(d_out)
    assert all_sent(got[words:]), case.name
    assert np.array_equal(zkgpu.from_device(d_f), f_img) and np.array_equal(zkgpu.from_device(d_t), t_img), case.name
    return got[:words]


@pytest.mark.parametrize("dim", [1, 3])
@pytest.mark.parametrize("n", hc.SIZES)
def test_multiset_diff_on_chains(zkgpu, n, dim):
    names = []
    for case in cases_4n(n, dim):
        want = mc.out_words(mc.reference(case.f, case.t, MAX_VALS), MAX_VALS)
        first, again = run_multiset(zkgpu, case), run_multiset(zkgpu, case)
        assert np.array_equal(first, again), (case.name, "two runs differ")
        bad = np.nonzero(first != want)[0]
        assert bad.size == 0, (case.name, "first wrong word", int(bad[0]), first[bad[:6]], want[bad[:6]])
        names.append(case.name)
    assert set(names) >= {"same_slot", "miss_behind_chain_row0"} | ({"wrap", "dense_run"} if n >= 255 else set())


@pytest.mark.parametrize("dim", [1, 3])
@pytest.mark.parametrize("n", hc.SIZES)
def test_lookup_misses_on_chains(zkgpu, n, dim):
    for case in cases_4n(n, dim):
        ref = lc.reference(case.f, case.t, MAX_VALS)
        want = lc.out_words(ref, MAX_VALS)
        first, again = run_lookup(zkgpu, case), run_lookup(zkgpu, case)
        assert np.array_equal(first, again), (case.name, "two runs differ")
        bad = np.nonzero(first != want)[0]
        assert bad.size == 0, (case.name, "first wrong word", int(bad[0]), first[bad[:6]], want[bad[:6]])
        # what the construction promises: the absent keys, the first of them at the case's row
        n_abs = 0 if case.absent is None else case.absent.shape[1]
        assert ref[1] == n_abs and (ref[2][0][0] if n_abs else None) == case.miss, case.name
