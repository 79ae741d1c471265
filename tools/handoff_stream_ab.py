#!/usr/bin/env python3
"""The executor hand-off under stage 1 (zkgpu_stark_prove_from_rows): per
instance, one proof timed three ways -- (a) prove() with the trace resident,
(b) set_cm1 + prove(), the upload serial with the proof, (c) prove_from_rows,
the upload under stage 1 -- with the source page-locked, beside the H2D rate
of the window loader's strided block copies and of the contiguous loader, and
the stage-1 timers.  Host wall time around the calls (each returns with the
proof on the host), median of --reps after one warm run.

Instances: config-4 at 2^23 rows (resident plan) and the fork-9 zkEVM-shaped
instance at 2^23 under the lean plan (a 50.4 GB page-locked trace: skipped,
with the reason, when the host does not hold it).  One process; it ends itself
at --time-limit seconds and writes what it has after every step.  GPU box.

Usage: tools/handoff_stream_ab.py [--instances config4,fork9] [--log-n 23]
                                  [--reps 3] [--time-limit 1100] out.json
"""
import argparse
import json
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "zkevm-prover_amd")]


def timed(fn, reps, before=None):
    """[s] of reps calls after one warm call; before() runs untimed ahead of each"""
    import torch
    out = []
    for k in range(reps + 1):
        if before:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k:
            out.append(time.perf_counter() - t0)
    return out


def summary(ts):
    return {"s_median": round(statistics.median(ts), 4), "s": [round(t, 4) for t in ts]}


def h2d_rates(zkgpu, torch, rows, batches, reps):
    """the contiguous loader over the whole width against the streamed window
    loader (zkgpu_load_stream_*: strided block copies, one lane across the
    windows) over the same rows in windows of each width of `batches`; the
    pinned source as it is"""
    n, w = rows.shape
    res = {"bytes": int(rows.nbytes), "windows": {}}
    cols = torch.empty((w, n), dtype=torch.int64, device="cuda")
    stage = torch.empty(2 * min(n * 128, (64 << 20) // 8), dtype=torch.int64, device="cuda")  # as the prover's
    ts = timed(lambda: zkgpu.load_rows_dev(cols, n, rows), reps)
    res["contiguous"] = dict(summary(ts), **{"GB/s": round(rows.nbytes / statistics.median(ts) / 1e9, 1)})
    for batch in batches:
        if batch >= w:
            res["windows"][str(batch)] = "one window is the whole width: the contiguous copy"
            continue

        def windows():
            s = zkgpu.RowsStream(rows, stage)
            for c0 in range(0, w, batch):
                s.window(cols[c0], n, c0, min(batch, w - c0))
            s.close()
        ts = timed(windows, reps)
        res["windows"][str(batch)] = dict(summary(ts), **{"GB/s": round(rows.nbytes / statistics.median(ts) / 1e9, 1)})
    del cols, stage
    torch.cuda.empty_cache()
    return res


def measure(name, inst, mode, reps, dump):
    import numpy as np
    import torch
    import zkgpu
    from zkgpu.stark import GpuStark, slib
    n, w = 1 << inst.n_bits, inst.n_cm1
    res = {"rows": n, "cm1_cols": w, "trace_bytes": n * w * 8}
    dump(name, res)
    try:
        pinned = torch.empty((n, w), dtype=torch.int64, pin_memory=True)
    except RuntimeError as e:
        res["skipped"] = "the host does not hold the page-locked trace: %s" % str(e).split("\n")[0]
        return res
    rows = pinned.numpy().view(np.uint64)
    # the instance's own witness read back into the pinned buffer, so the lookups hold
    g = GpuStark(inst, mode=mode)
    g.witness()
    if slib().zkgpu_stark_get_cm1(g.h, pinned.data_ptr()):
        raise RuntimeError(slib().zkgpu_stark_last_error().decode())
    lean = g.memory_mode() == "lean"
    res["plan"] = g.memory_mode()
    res["stream_batch_cols"] = 128 if w >= 256 else 64  # the prover's default (host/starks.cpp stream_batch_cols)
    sweep = [b for b in (128, 64, 32, 16) if b < w and b != res["stream_batch_cols"]]
    if lean:  # the rate probe's columns do not fit beside the lean arena
        g.close()
        torch.cuda.empty_cache()
    res["h2d"] = h2d_rates(zkgpu, torch, rows, [res["stream_batch_cols"]] + sweep, 2)
    dump(name, res)
    if lean:
        g = GpuStark(inst, mode=mode)
    ref = [None]

    def prove():
        p = g.prove_raw()
        ref[0] = p if ref[0] is None else ref[0]
        assert np.array_equal(p, ref[0]), "prove() differs between runs"

    def stream():
        assert np.array_equal(g.prove_from_rows_raw(pinned.data_ptr()), ref[0]), "prove_from_rows != prove"

    def serial():
        g.set_cm1(rows)
        prove()

    a = timed(prove, reps, before=(lambda: g.set_cm1(rows)) if lean else None)
    t = g.timers()
    res["a_prove_resident"] = dict(summary(a), stage1_ms={k: round(v, 2) for k, v in t.items() if "STEP_1" in k})
    dump(name, res)
    res["b_set_cm1_then_prove"] = summary(timed(serial, reps))
    dump(name, res)
    c = timed(stream, reps)
    t = g.timers()
    res["c_prove_from_rows"] = dict(summary(c), stage1_ms={k: round(v, 2) for k, v in t.items() if "STEP_1" in k})
    res["c_over_a"] = round(statistics.median(c) / statistics.median(a), 3)
    res["b_over_a"] = round(res["b_set_cm1_then_prove"]["s_median"] / statistics.median(a), 3)
    res["target"] = "c <= 1.15 a (reported against, not a gate)"
    # (c) against the batch width (ZKGPU_STREAM_COLS; the default above)
    res["c_by_stream_cols"] = {}
    for b in sweep:
        os.environ["ZKGPU_STREAM_COLS"] = str(b)
        try:
            ts = timed(stream, reps)
        finally:
            del os.environ["ZKGPU_STREAM_COLS"]
        res["c_by_stream_cols"][str(b)] = dict(summary(ts), stage1_stream_ms=round(g.timers()["STARK_STEP_1_STREAM"], 2),
                                               c_over_a=round(statistics.median(ts) / statistics.median(a), 3))
        dump(name, res)
    g.close()
    del pinned, rows
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", default="config4,fork9")
    ap.add_argument("--log-n", type=int, default=23)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--time-limit", type=int, default=1100)
    ap.add_argument("out")
    args = ap.parse_args()
    import bench
    import zkgpu
    from zkgpu import stamp
    from zkgpu.stark import MEM_AUTO, MEM_LEAN
    doc = {"what": __doc__.split("\n\n")[0], "stamps": stamp.all_stamps(), "reps": args.reps, "instances": {}}

    def dump(name, res):
        doc["instances"][name] = res
        with open(args.out + ".tmp", "w") as f:
            json.dump(doc, f, indent=1)
        os.replace(args.out + ".tmp", args.out)

    def out_of_time(*_):
        doc["ended"] = "the process's own time limit (%d s)" % args.time_limit
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
        os._exit(3)

    signal.signal(signal.SIGALRM, out_of_time)
    signal.alarm(args.time_limit)
    zkgpu.init(0)
    todo = {"config4": (lambda: bench.stark_instance(args.log_n, 1, 100, 128), MEM_AUTO),
            "fork9": (lambda: bench.stark_instance(args.log_n, 1, 100, 128, "zkevm"), MEM_LEAN)}
    for name in args.instances.split(","):
        make, mode = todo[name]
        res = measure(name, make(), mode, args.reps, dump)
        dump(name, res)
        print(name, json.dumps(res), flush=True)
    signal.alarm(0)


if __name__ == "__main__":
    main()
