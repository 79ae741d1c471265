#!/usr/bin/env python3
"""What a trace audit (zkgpu_stark_audit) costs beside a proof of the same
handle: per case one process, one prover, the kernels warmed, then an audit and
a proof alternating on the same loaded trace.  Reported per case: the audit's
AUDIT_* timer lines and its wall time, the proof's wall time and STARK_TOTAL
(median and range over the repeats), what the audit found and, for a trace with
a finding, the message the proof ends with -- the one finding a developer gets
from a proof today, and what it costs to get it.

Cases: config-4 at 2^23 rows, clean and with one finding per layer -- an
identity broken on one row, one plookup source cell set to a value its table
does not hold, and (the same instance with one permutation check added: config-4
has none) one permutation cell altered --, and the north-star instance, the
fork-9 zkEVM-shaped one under the lean plan, where every row fails the stand-in
AIR, with naming off and on.  Under the lean plan the trace is loaded before
every audit + proof pair (the proof consumes it; the audit does not).  There is
no threshold: the figures are a record.  It ends itself at --time-limit seconds
and writes what it has after every step.  GPU box.

Usage: tools/audit_cost.py [--cases config4,config4_perm,fork9] [--log-n 23]
                           [--reps 5] [--time-limit 1100] out.json
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

P = 0xFFFFFFFF00000001
ABSENT = 12345  # the tables hold pseudo-random 63-bit values: the audit's report confirms the miss


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3),
            "all": [round(x, 3) for x in xs]}


def findings(r):
    """the report without its challenges and values: what was found"""
    return {"clean": r["clean"], "n_pu_bad": r["n_pu_bad"],
            "pu": [(e["pu"], e["n_rows"], e["n_vals"]) for e in r["pu"]], "n_z_open": r["n_z_open"],
            "z": [(e["z"], e["n_num"], e["n_den"]) for e in r["z"]],
            "identities": {k: r["identities"][k] for k in ("ran", "n_bad")},
            "first_rows": r["identities"]["rows"][:4]}


def alternate(g, reps, names, load, dump, res):
    """audit, then proof, of the same loaded trace, `reps` times after one warming pair"""
    from zkgpu import ZkgpuError
    lines, audit_wall, proof_wall, proof_total = {}, [], [], []
    for rep in range(reps + 1):
        load()
        t0 = time.perf_counter()
        r = g.audit(names=names)
        t1 = time.perf_counter()
        t = g.timers()
        try:
            g.prove_raw()
            total = g.timers()["STARK_TOTAL"]
            res["proof"] = "succeeds"
        except ZkgpuError as e:
            total = None
            res["proof"] = "fails: " + str(e)[:300]
        t2 = time.perf_counter()
        res["found"] = findings(r)
        if rep == 0:
            continue  # warm: the kernels compiled or loaded, the workspaces grown
        for k, v in t.items():
            lines.setdefault(k, []).append(v)
        audit_wall.append((t1 - t0) * 1e3)
        proof_wall.append((t2 - t1) * 1e3)
        if total is not None:
            proof_total.append(total)
        res["audit_ms"] = {k: spread(v) for k, v in lines.items()}
        res["audit_wall_ms"] = spread(audit_wall)
        res["proof_wall_ms"] = spread(proof_wall)
        if proof_total:
            res["proof_STARK_TOTAL_ms"] = spread(proof_total)
        res["audit_over_proof_wall"] = round(res["audit_wall_ms"]["median"] / res["proof_wall_ms"]["median"], 4)
        dump()


def measure(inst, mode, reps, dump, plan):
    """plan: [(case name, names, fault)] with fault None or a function (inst, trace) -> [(row, col, value)]"""
    from zkgpu.stark import GpuStark
    g = GpuStark(inst, mode=mode)
    lean = g.memory_mode() == "lean"
    out = {"rows": 1 << inst.n_bits, "plan": g.memory_mode(), "cases": {}}
    dump(out)
    g.witness()
    trace = None
    for name, names, fault in plan:
        res = out["cases"][name] = {"names": bool(names)}
        if fault is None:
            load = g.witness if lean else (lambda: None)
            if not lean and trace is not None:
                g.set_cm1(trace)
        else:
            if lean:
                raise ValueError("faults are planted in a resident trace")
            if trace is None:
                trace = g.get_cm1()
            cells = fault(inst, trace)
            keep = [(r, c, int(trace[r, c])) for r, c, _ in cells]
            for r, c, v in cells:
                trace[r, c] = v
            g.set_cm1(trace)
            for r, c, v in keep:
                trace[r, c] = v
            res["cells"] = [(r, c) for r, c, _ in cells]
            load = lambda: None  # noqa: E731  (resident: a failed proof leaves the trace)
        alternate(g, reps, names, load, lambda: dump(out), res)
    g.close()
    return out


def identity_fault(inst, trace):
    row = (1 << inst.n_bits) // 2 + 1
    return [(row, 2, (int(trace[row, 2]) + 1) % P)]


def lookup_fault(inst, trace):
    row = (1 << inst.n_bits) // 3
    return [(row, inst.cm1_lk[2], ABSENT)]  # plookup 1's source column C


def perm_fault(inst, trace):
    row = (1 << inst.n_bits) // 5
    c = inst.perms[0]["cols"][2]
    return [(row, c, (int(trace[row, c]) + 1) % P)]


def config4_perm(log_n):
    """bench.stark_instance's config-4 arguments with one permutation check added"""
    from zkgpu.synthetic import SyntheticStark
    import bench
    base = bench.stark_instance(log_n, 1, 100, 128)
    t = (100 - 3) // 3
    return SyntheticStark(n_bits=log_n, blowup_bits=1, t=t, n_free=100 - 3 - 3 * t, m=6, n_k=26, n_queries=128,
                          fri_steps=base.fri_steps, n_lookups=2, n_perms=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="config4,config4_perm,fork9")
    ap.add_argument("--log-n", type=int, default=23)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--time-limit", type=int, default=1100)
    ap.add_argument("out")
    args = ap.parse_args()
    import bench
    import zkgpu
    from zkgpu import stamp
    from zkgpu.stark import MEM_AUTO, MEM_LEAN
    doc = {"what": " ".join(__doc__.split("\n\n")[0].split()), "stamps": stamp.all_stamps(), "reps": args.reps,
           "instances": {}}

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
    todo = {
        "config4": (lambda: bench.stark_instance(args.log_n, 1, 100, 128), MEM_AUTO,
                    [("clean", True, None), ("identity_one_row", True, identity_fault),
                     ("plookup_one_cell", True, lookup_fault)]),
        "config4_perm": (lambda: config4_perm(args.log_n), MEM_AUTO,
                         [("clean", True, None), ("permutation_one_cell", True, perm_fault)]),
        "fork9": (lambda: bench.stark_instance(args.log_n, 1, 100, 128, "zkevm"), MEM_LEAN,
                  [("every_row_fails_names_off", False, None), ("every_row_fails_names_on", True, None)]),
    }
    for name in args.cases.split(","):
        make, mode, plan = todo[name]

        def dump(res, name=name):
            doc["instances"][name] = res
            write()
        res = measure(make(), mode, args.reps, dump, plan)
        dump(res)
        print(name, json.dumps(res), flush=True)
    signal.alarm(0)


if __name__ == "__main__":
    main()
