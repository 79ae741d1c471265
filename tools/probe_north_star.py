#!/usr/bin/env python3
"""The north-star proof (the fork-9 zkEVM-shaped instance at 2^23 rows, lean
HBM plan) with a probe (include/zkgpu_stark.h zkgpu_stark_probe_*): sampled
rows of every section around each of the five stage programs, re-evaluated
from the ZXP source programs (tests/zxp_rows.py check_probe) -- the stage-2/3
outputs, q_2ns and the FRI polynomial on a proof's own data at the timed size,
under the aliasing only the lean plan at that size has.

One process: the instance, one untimed proof (the process's first loads the
compiled programs), one proof without a probe, one with, the check.
Sampled rows: tests/test_oracle_rows.sample_rows per domain (first / last
rows, both sides of every power of two >= 2^8, --n-random random rows; at most
2048 per domain).  The lean plan's keep_cols boundary and the streamed stage
1's 128-column batch boundaries are column boundaries: every record covers its
section's whole width, which the output states per boundary (the trace is
generated on the device, so the streamed stage 1 itself is not run here:
tests/test_gpu_probe.py probes it at 2^10).

Writes per point the rows and columns compared, the mismatches (must be 0),
both proofs' s/proof from the prover's own STARK_TOTAL timer, the probe's
read-back, and zkgpu.stamp.all_stamps().  GPU box; ends itself at --time-limit.

Usage: tools/probe_north_star.py [--log-n 23] [--n-random 1024] [--time-limit 900]
                                 [--out profiles/r08_probe_north_star.json]
"""
import argparse
import json
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "zkevm-prover_amd"), os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=23)
    ap.add_argument("--n-random", type=int, default=1024)
    ap.add_argument("--queries", type=int, default=128)
    ap.add_argument("--time-limit", type=int, default=900)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_probe_north_star.json"))
    args = ap.parse_args()
    signal.alarm(args.time_limit)

    import numpy as np
    import bench
    import zkgpu
    import zkgpu.stamp
    import zxp_rows as zr
    from test_oracle_rows import sample_rows
    from zkgpu.stark import GpuStark, MEM_LEAN

    zkgpu.init(0)
    inst = bench.stark_instance(args.log_n, 1, 100, args.queries, "zkevm")
    rng = np.random.default_rng(23)
    rows = [sample_rows(1 << b, rng, n_random=args.n_random)[0] for b in (inst.n_bits, inst.n_bits_ext)]
    assert all(r.size <= 2048 for r in rows), [r.size for r in rows]
    doc = {"instance": {"kind": "zkevm", "n_bits": inst.n_bits, "n_bits_ext": inst.n_bits_ext,
                        "widths": [inst.n_cm1, inst.n_cm2, inst.n_cm3, inst.n_cm4], "queries": args.queries},
           "memory_plan": "lean", "sampled_rows": {"n": int(rows[0].size), "ext": int(rows[1].size)},
           "stamps": zkgpu.stamp.all_stamps()}
    t_start = t0 = time.perf_counter()

    def say(what):
        print("[%7.1f s] %s" % (time.perf_counter() - t_start, what), file=sys.stderr, flush=True)

    g = GpuStark(inst, mode=MEM_LEAN)
    try:
        assert g.memory_mode() == "lean"
        doc["setup_s"] = round(time.perf_counter() - t0, 2)
        g.witness()
        say("set up; one untimed proof (the process's first loads the compiled programs)")
        g.prove_raw()
        doc["first_proof_s"] = round(g.timers()["STARK_TOTAL"] / 1e3, 4)
        g.witness()
        say("proving without a probe")
        plain = g.prove_raw()
        t_plain = g.timers()
        say("proving with a probe")
        g.probe_set(rows[0], rows[1])
        g.witness()
        probed = g.prove_raw()
        t_probed = g.timers()
        doc["proofs_identical"] = bool(np.array_equal(plain, probed))
        doc["s_per_proof"] = {"no_probe": round(t_plain["STARK_TOTAL"] / 1e3, 4),
                              "probe": round(t_probed["STARK_TOTAL"] / 1e3, 4)}
        doc["probe_readback_ms"] = round(t_probed["ZKGPU_PROBE_READBACK"], 2)
        n_recs, n_words = g.probe_size()
        doc["probe"] = {"records": n_recs, "payload_MB": round(n_words * 8 / 1e6, 1)}
        probe = g.probe()
        publics = g.publics()
    finally:
        g.close()
    # the column boundaries of the lean plan: inside whole-width records of cm1
    cm1 = {zr.POINT_NAMES[p]: int(v.shape[1]) for p, a, s, _, v in probe if s in (0, zr.SEC_CM1_2NS) and not a}
    batches = list(range(128, inst.n_cm1, 128))
    doc["column_boundaries"] = {
        "stage1": "lean plan, trace generated on the device (witness): the streamed stage 1 itself is not run here",
        "cm1_records_ncols": cm1, "n_cm1": inst.n_cm1, "stream_batch_boundaries": batches,
        "stream_batch_boundaries_present": bool(cm1) and all(w == inst.n_cm1 for w in cm1.values()),
        "keep_cols_boundary_present": "cm1_2ns at step42ns" if cm1.get("step42ns") == inst.n_cm1 else False}
    say("checking %d records" % len(probe))
    t0 = time.perf_counter()
    stats = {}
    bad = zr.check_probe(inst, probe, publics, stats)
    doc["check_s"] = round(time.perf_counter() - t0, 1)
    doc["compared"] = {zr.POINT_NAMES[p]: {"rows": s["rows"], "cols": s["cols"], "nonzero": s["nonzero"]}
                       for p, s in sorted(stats.items())}
    doc["mismatches"] = len(bad)
    doc["first_mismatches"] = [list(b) for b in bad[:20]]
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({k: doc[k] for k in ("s_per_proof", "probe_readback_ms", "compared", "mismatches",
                                          "proofs_identical")}))
    return 0 if not bad and doc["proofs_identical"] and len(stats) == 5 else 1


if __name__ == "__main__":
    sys.exit(main())
