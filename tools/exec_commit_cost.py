#!/usr/bin/env python3
"""What the circom .exec hand-off costs on the GPU (zkgpu_stark_set_cm1_witness)
beside the two ways a trace got into cm1_n before it, at a C12a-like shape:
2^22 rows x 12 committed columns.

The real circuits' .exec files are not in the repository, so the images here
are SYNTHETIC GUESSES: size_witness, the number of adds and the depth of the
add DAG are swept over a stated grid (GRID below), every level of a shape is
equally wide, an add reads one slot of the level before it and one witness
slot, nine sMap cells in ten read a random slot and the tenth is empty.

Per shape, wall time of a call (median and range over the repeats, after two
warm-up calls):
  set_cm1_witness        witness -> cm1_n through the planned hand-off
  set_cm1                zkgpu_stark_set_cm1 of the finished n x 12 rows: the
                         only way in before (the host loop that makes the rows
                         is NOT in this figure, so the comparison is conservative)
  host_loop              a single-thread C++ restatement of the reference's loop
                         (main.recursive1.cpp:343-394; compiled by the tool with
                         g++ -O2), witness -> the n x 12 row-major rows
  host_loop_plus_set_cm1 the sum of the two medians: what an integrator ran
with n_levels / n_launches of the plan and its device bytes.  The hand-off's
cm1_n is compared with the host loop's rows once per shape.  One A/B of the
tail width T (256 / 1024) on the deep-chain shape.  GPU box.

Usage: tools/exec_commit_cost.py [--log-n 22] [--reps 10] out.json
"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "zkevm-prover_amd")]

P = 0xFFFFFFFF00000001
N_COLS = 12
# (size_witness, nAdds, depth): every level nAdds / depth adds wide
GRID = [(1 << 20, 1 << 20, 16), (1 << 20, 1 << 20, 2048), (1 << 20, 1 << 22, 64),
        (1 << 23, 1 << 20, 16), (1 << 23, 1 << 20, 2048), (1 << 23, 1 << 22, 64)]
DEEP_CHAIN = (1 << 20, 1 << 20, 2048)  # levels of 512 adds: one workgroup launch at T = 1024, 2048 grid launches at 256
SOURCES = ["csrc/exec.hip", "csrc/exec_plan.cpp", "csrc/exec_plan.hpp", "csrc/gl_device.hpp"]

HOST_LOOP = r"""
#include <stdint.h>
static const uint64_t P = 0xFFFFFFFF00000001ULL, EPS = 0xFFFFFFFFULL;
static inline uint64_t red(unsigned __int128 x)
{
    const uint64_t lo = (uint64_t)x, hi = (uint64_t)(x >> 64), hh = hi >> 32, hl = hi & EPS;
    uint64_t t, r;
    if (__builtin_sub_overflow(lo, hh, &t)) t -= EPS;
    if (__builtin_add_overflow(t, hl * EPS, &r)) r += EPS;
    return r;
}
static inline uint64_t add(uint64_t a, uint64_t b)
{
    uint64_t s;
    if (__builtin_add_overflow(a, b, &s) && __builtin_add_overflow(s, EPS, &s)) s += EPS;
    return s;
}
extern "C" void exec_host_loop(uint64_t *rows, uint64_t *tmp, const uint64_t *image, const uint64_t *witness,
                               uint64_t size_witness, uint64_t n_cols, uint64_t n)
{
    const uint64_t n_adds = image[0], n_smap = image[1], *adds = image + 2, *smap = adds + 4 * n_adds;
    for (uint64_t i = 0; i < size_witness; i++) tmp[i] = witness[i];
    for (uint64_t i = 0; i < n_adds; i++) {
        const uint64_t *a = adds + 4 * i;
        const uint64_t v = add(red((unsigned __int128)tmp[a[0]] * a[2]), red((unsigned __int128)tmp[a[1]] * a[3]));
        tmp[size_witness + i] = v >= P ? v - P : v;
    }
    for (uint64_t i = 0; i < n_smap; i++)
        for (uint64_t j = 0; j < n_cols; j++) {
            const uint64_t s = smap[n_cols * i + j], v = s ? tmp[s] : 0;
            rows[i * n_cols + j] = v >= P ? v - P : v;
        }
    for (uint64_t k = n_smap * n_cols; k < n * n_cols; k++) rows[k] = 0;
}
"""


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def timed(call, reps, warm=2):
    for _ in range(warm):
        call()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return spread(ms)


def source_stamp():
    h = hashlib.sha256()
    for rel in SOURCES:
        h.update(rel.encode())
        with open(os.path.join(ROOT, "zkevm-prover_amd", rel), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def host_loop_lib(d):
    src, so = os.path.join(d, "exec_host_loop.cpp"), os.path.join(d, "exec_host_loop.so")
    with open(src, "w") as f:
        f.write(HOST_LOOP)
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", so, src])
    L = ctypes.CDLL(so)
    L.exec_host_loop.restype = None
    L.exec_host_loop.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_uint64] * 3
    return L


def synthetic(np, rng, sw, n_adds, depth, n):
    """-> (witness, image): `depth` levels of n_adds / depth adds each"""
    w = n_adds // depth
    i = np.arange(n_adds, dtype=np.uint64)
    lev = i // np.uint64(w)
    prev = np.uint64(sw) + (lev - np.uint64(1)) * np.uint64(w) + rng.integers(0, w, size=n_adds, dtype=np.uint64)
    adds = np.empty((n_adds, 4), np.uint64)
    adds[:, 0] = np.where(lev == 0, rng.integers(0, sw, size=n_adds, dtype=np.uint64), prev)
    adds[:, 1] = rng.integers(0, sw, size=n_adds, dtype=np.uint64)
    adds[:, 2:] = rng.integers(0, 2**64, size=(n_adds, 2), dtype=np.uint64)
    smap = rng.integers(0, sw + n_adds, size=(n, N_COLS), dtype=np.uint64)
    smap[rng.random((n, N_COLS)) < 0.1] = 0
    image = np.concatenate([np.array([n_adds, n], np.uint64), adds.reshape(-1), smap.reshape(-1)])
    witness = rng.integers(0, 2**64, size=sw, dtype=np.uint64)
    witness[0] = 1
    return witness, image


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=22)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("out")
    args = ap.parse_args()
    import numpy as np
    import torch
    import zkgpu
    from zkgpu.stark import GpuStark, MEM_RESIDENT
    from zkgpu.synthetic import SyntheticStark
    zkgpu.init()
    n = 1 << args.log_n
    inst = SyntheticStark(n_bits=args.log_n, t=4, m=2, n_lookups=0)
    assert inst.n_cm1 == N_COLS
    g = GpuStark(inst, mode=MEM_RESIDENT)
    rng = np.random.default_rng(11)
    res = {"note": "SYNTHETIC shapes: the real .exec files are absent, size_witness / nAdds / depth are guesses "
                   "swept over `grid`; set_cm1 leaves out the host loop that makes its rows",
           "rows": n, "n_cols": N_COLS, "reps": args.reps, "host_loop_reps": args.host_reps,
           "grid": [list(s) for s in GRID], "source_stamp": source_stamp(), "sources": SOURCES, "shapes": []}
    rows = np.empty((n, N_COLS), np.uint64)
    with tempfile.TemporaryDirectory() as d:
        L = host_loop_lib(d)

        def measure(shape, tail):
            sw, n_adds, depth = shape
            witness, image = synthetic(np, rng, sw, n_adds, depth, n)
            tmp = np.empty(sw + n_adds, np.uint64)
            zkgpu.exec_set_tail_width(tail)
            t0 = time.perf_counter()
            g.set_exec(image, sw)
            plan_ms = (time.perf_counter() - t0) * 1e3
            ex = zkgpu.Exec(image, sw, N_COLS)  # the same plan once more, for its figures
            info = ex.info()
            ex.close()
            zkgpu.exec_set_tail_width(0)
            out = {"size_witness": sw, "n_adds": n_adds, "depth": depth, "tail_width": tail or 1024,
                   "n_levels": info["n_levels"], "n_launches": info["n_launches"], "device_bytes": info["device_bytes"],
                   "set_exec_ms": round(plan_ms, 1),
                   "set_cm1_witness_ms": timed(lambda: g.set_cm1_witness(witness), args.reps)}

            def host():
                L.exec_host_loop(rows.ctypes.data, tmp.ctypes.data, image.ctypes.data, witness.ctypes.data, sw, N_COLS, n)
            out["host_loop_ms"] = timed(host, args.host_reps, warm=1)
            assert np.array_equal(g.get_cm1(), rows), "the hand-off differs from the host loop"
            out["set_cm1_ms"] = timed(lambda: g.set_cm1(rows), args.reps)
            out["host_loop_plus_set_cm1_ms"] = round(out["host_loop_ms"]["median"] + out["set_cm1_ms"]["median"], 3)
            return out

        for shape in GRID:
            res["shapes"].append(measure(shape, 0))
            print(json.dumps(res["shapes"][-1]), flush=True)
        res["tail_width_ab_deep_chain"] = [measure(DEEP_CHAIN, t) for t in (256, 1024)]
    g.close()
    res["device"] = torch.cuda.get_device_name(0)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
