#!/usr/bin/env python3
"""What the calculateZ diagnosis costs on its failing path: the multiset
comparison (zkgpu_multiset_diff_dev) of one column pair of dimension 3 that
differs in one value, beside zkgpu_h1h2_dev -- the nearest existing work of the
same shape (one hash table over the same rows) -- at the same size in the same
process.  Per call: wall time around a stream synchronisation (median and
spread over the repeats, after two warm-up calls that grow the workspace) and
the per-kernel event times of the comparison.  Also: the comparison when one
default value sits on every row but one (the flipped-selector shape).  GPU box.

Usage: tools/z_diag_cost.py [--log-n 23] [--reps 10] out.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "zkevm-prover_amd")]

P = 0xFFFFFFFF00000001
KERNELS = ("k_multiset_insert", "k_multiset_flag", "k_nz_count", "k_nz_emit", "k_multiset_emit")


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def timed(zkgpu, call, reps):
    for _ in range(2):
        call()
    zkgpu.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        zkgpu.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return spread(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=23)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("out")
    args = ap.parse_args()
    import numpy as np
    import torch
    import zkgpu
    zkgpu.init()
    n, dim = 1 << args.log_n, 3
    rng = np.random.default_rng(7)
    a = rng.integers(0, P, size=(dim, n), dtype=np.uint64)
    b = a[:, rng.permutation(n)]
    b[0, n // 2] ^= np.uint64(1)
    d_a, d_b = zkgpu.to_device(a), zkgpu.to_device(b)
    out = torch.zeros(2 * (1 + 3 * 16), dtype=torch.int64, device="cuda:0")
    h1, h2 = torch.zeros(dim * n, dtype=torch.int64, device="cuda:0"), torch.zeros(dim * n, dtype=torch.int64,
                                                                                 device="cuda:0")
    res = {"rows": n, "dim": dim, "reps": args.reps, "max_vals": 16,
           "workspace_bytes": zkgpu.multiset_diff_workspace_bytes(n)}

    def diff(x, y):
        return lambda: zkgpu.multiset_diff_dev(out, x, n, y, n, n, dim, 16)

    res["multiset_diff_ms"] = timed(zkgpu, diff(d_a, d_b), args.reps)
    got = zkgpu.from_device(out)
    assert (got[0], got[49]) == (1, 1) and (got[2], got[3]) == (1, 0), got[:8]
    res["multiset_diff_result"] = {"n_a": int(got[0]), "first_a": [int(x) for x in got[1:4]], "n_b": int(got[49]),
                                   "first_b": [int(x) for x in got[50:53]]}
    zkgpu.prof_enable(True)
    zkgpu.prof_reset()
    diff(d_a, d_b)()
    zkgpu.synchronize()
    res["multiset_diff_kernels_ms"] = {k: round(zkgpu.prof_query(k)[1], 3) for k in KERNELS}
    zkgpu.prof_enable(False)
    # the parent's plookup on columns of the same shape: f a permutation of t (every value included)
    d_t = zkgpu.to_device(a)
    d_f = zkgpu.to_device(a[:, rng.permutation(n)])
    res["h1h2_ms"] = timed(zkgpu, lambda: zkgpu.h1h2_dev(h1, n, h2, n, d_f, n, d_t, n, n, dim), args.reps)
    # one default value on every row but one of a, on every row of b: all rows contend on one slot
    s = np.repeat(a[:, :1], n, axis=1)
    d_sb = zkgpu.to_device(s)
    s[:, n // 3] = a[:, 1]
    d_sa = zkgpu.to_device(s)
    res["multiset_diff_selector_ms"] = timed(zkgpu, diff(d_sa, d_sb), args.reps)
    got = zkgpu.from_device(out)
    assert (got[0], got[49]) == (2, 1) and tuple(got[1:4]) == (0, n - 1, n), got[:8]
    res["device"] = torch.cuda.get_device_name(0)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
