#!/usr/bin/env python3
"""What the constraint check (zkgpu_stark_check_set) adds to a proof: per
instance, one process, one prover, the kernels warmed, then proofs alternating
check OFF and REPORT on the same trace.  Reported per mode: STARK_TOTAL (median
and spread over the repeats), and for the checked proofs the
ZKGPU_CHECK_CONSTRAINTS line beside the quotient line
(STARK_STEP_4_CALCULATE_EXPS_2NS) of the same proofs.  Every checked proof must
equal the unchecked one; the count of failing rows is recorded.

Instances: config-4 at 2^23 rows (plan chosen by the prover) and the fork-9
zkEVM-shaped instance at 2^23 under the lean plan (the trace is loaded before
every proof: the lean plan consumes it).  The first checked proof compiles the
check's kernels (not timed).  It ends itself at --time-limit seconds and writes
what it has after every step.  GPU box.

With --names the question is what naming (zkgpu_stark_check_names_set) adds to
a checked proof instead: REPORT with naming off and on alternating on a clean
trace -- the yardstick is naming off in the same process --, then once on a
trace with one broken row.

Usage: tools/constraint_check_ab.py [--instances config4,fork9] [--log-n 23]
                                    [--reps 5] [--time-limit 1100] [--names] out.json
"""
import argparse
import json
import os
import signal
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "zkevm-prover_amd")]

CHECK, QUOTIENT = "ZKGPU_CHECK_CONSTRAINTS", "STARK_STEP_4_CALCULATE_EXPS_2NS"


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3),
            "all": [round(x, 3) for x in xs]}


def measure(inst, mode, reps, dump):
    import numpy as np
    from zkgpu.stark import CHECK_OFF, CHECK_REPORT, GpuStark
    g = GpuStark(inst, mode=mode)
    lean = g.memory_mode() == "lean"
    res = {"rows": 1 << inst.n_bits, "plan": g.memory_mode()}
    ref = [None]
    lines = {CHECK_OFF: {"STARK_TOTAL": [], QUOTIENT: []}, CHECK_REPORT: {"STARK_TOTAL": [], QUOTIENT: [], CHECK: []}}

    def prove(check, keep):
        g.check_set(check)
        if lean or ref[0] is None:
            g.witness()
        p = g.prove_raw()
        ref[0] = p if ref[0] is None else ref[0]
        assert np.array_equal(p, ref[0]), "a checked proof differs from the unchecked one"
        if check:
            r = g.check_result()
            assert r["ran"] == 1, r
            res["n_bad"] = r["n_bad"]  # (the zkEVM-shaped instance is no satisfiable AIR: every row fails)
        t = g.timers()
        assert (CHECK in t) == bool(check)
        if keep:
            for k in lines[check]:
                lines[check][k].append(t[k])

    for check in (CHECK_OFF, CHECK_REPORT):  # warm: the kernels compiled or loaded, the workspaces grown
        prove(check, False)
    for _ in range(reps):
        for check in (CHECK_OFF, CHECK_REPORT):
            prove(check, True)
        res["off_ms"] = {k: spread(v) for k, v in lines[CHECK_OFF].items()}
        res["report_ms"] = {k: spread(v) for k, v in lines[CHECK_REPORT].items()}
        dump(res)
    off, rep = res["off_ms"]["STARK_TOTAL"], res["report_ms"]["STARK_TOTAL"]
    res["total_report_minus_off_ms"] = round(rep["median"] - off["median"], 3)
    res["check_over_quotient"] = round(res["report_ms"][CHECK]["median"] / res["report_ms"][QUOTIENT]["median"], 4)
    g.close()
    return res


def measure_names(inst, mode, reps, dump):
    """What naming (zkgpu_stark_check_names_set) adds to a checked proof: REPORT with naming off and
    on alternating on a clean trace, the yardstick being naming off in the same process; then the same
    once over on a trace with one broken row (resident plans only: the trace is edited in place)."""
    import numpy as np
    from zkgpu.stark import CHECK_REPORT, GpuStark
    g = GpuStark(inst, mode=mode)
    lean = g.memory_mode() == "lean"
    res = {"rows": 1 << inst.n_bits, "plan": g.memory_mode()}
    g.check_set(CHECK_REPORT)
    ref = [None]

    def prove(names, lines, trace=None):
        g.check_names_set(names)
        if trace is not None:
            g.set_cm1(trace)
        elif lean or ref[0] is None:
            g.witness()
        p = g.prove_raw()
        if trace is None:
            ref[0] = p if ref[0] is None else ref[0]
            assert np.array_equal(p, ref[0]), "naming changed the proof"
        r = g.check_result()
        t = g.timers()
        if lines is not None:
            for k in lines:
                lines[k].append(t[k])
        return r

    def alternate(key, trace=None):
        lines = {n: {"STARK_TOTAL": [], CHECK: []} for n in (False, True)}
        for names in (False, True):
            prove(names, None, trace)
        for _ in range(reps):
            for names in (False, True):
                r = prove(names, lines[names], trace)
            res[key] = {"n_bad": r["n_bad"], "names_off_ms": {k: spread(v) for k, v in lines[False].items()},
                        "names_on_ms": {k: spread(v) for k, v in lines[True].items()}}
            dump(res)
        off, on = res[key]["names_off_ms"]["STARK_TOTAL"], res[key]["names_on_ms"]["STARK_TOTAL"]
        res[key]["on_median_within_off_range"] = bool(off["min"] <= on["median"] <= off["max"])
        res[key]["total_on_minus_off_ms"] = round(on["median"] - off["median"], 3)
        res[key]["check_on_minus_off_ms"] = round(res[key]["names_on_ms"][CHECK]["median"] -
                                                  res[key]["names_off_ms"][CHECK]["median"], 3)
        dump(res)

    res["n_terms"] = None
    alternate("clean")
    res["n_terms"] = int(g.check_terms().shape[0])
    if not lean:
        trace = g.get_cm1()
        row = (1 << inst.n_bits) // 2 + 1
        trace[row, 2] = (int(trace[row, 2]) + 1) % 0xFFFFFFFF00000001
        reps = 1  # (recorded once)
        alternate("one_broken_row", trace)
        res["one_broken_row"]["named"] = g.check_named(0)[0]
    g.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", default="config4,fork9")
    ap.add_argument("--log-n", type=int, default=23)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--time-limit", type=int, default=1100)
    ap.add_argument("--names", action="store_true", help="measure naming on against naming off (both REPORT)")
    ap.add_argument("out")
    args = ap.parse_args()
    import bench
    import zkgpu
    from zkgpu import stamp
    from zkgpu.stark import MEM_AUTO, MEM_LEAN
    what = " ".join(measure_names.__doc__.split()) if args.names else __doc__.split("\n\n")[0]
    doc = {"what": what, "stamps": stamp.all_stamps(), "reps": args.reps, "instances": {}}

    def write():
        with open(args.out + ".tmp", "w") as f:
            json.dump(doc, f, indent=1)
        os.replace(args.out + ".tmp", args.out)

    def out_of_time(*_):
        doc["ended"] = "the process's own time limit (%d s)" % args.time_limit
        write()
        os._exit(3)

    signal.signal(signal.SIGALRM, out_of_time)
    signal.alarm(args.time_limit)
    zkgpu.init(0)
    todo = {"config4": (lambda: bench.stark_instance(args.log_n, 1, 100, 128), MEM_AUTO),
            "fork9": (lambda: bench.stark_instance(args.log_n, 1, 100, 128, "zkevm"), MEM_LEAN)}
    for name in args.instances.split(","):
        make, mode = todo[name]

        def dump(res, name=name):
            doc["instances"][name] = res
            write()
        res = (measure_names if args.names else measure)(make(), mode, args.reps, dump)
        dump(res)
        print(name, json.dumps(res), flush=True)
    signal.alarm(0)


if __name__ == "__main__":
    main()
