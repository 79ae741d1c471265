#!/usr/bin/env python3
"""What naming the cells of a connection check costs (zkgpu_conn_breaks_dev,
zkgpu_stark_conn_check, layer B of zkgpu_stark_audit).

primitive  zkgpu_conn_breaks_dev alone at the recursion circuits' shape, 2^22
           rows x 12 columns, and at 2^23 x 2: a clean wiring (column i + 1 is
           column i rotated, the cycle closed through column 0) and the same
           with one cell off, the median of --reps calls after one warming
           call, wall time around a synchronisation and the kernels' own times
           (zkgpu_prof_query), beside the workspace bytes.
audit      the SyntheticStark instance with one connection at 2^20 rows: an
           audit of the clean trace and of the trace with one cell off, each
           with the connection declared and undeclared.  The undeclared audit
           is the code path of an audit before connections existed, so the
           kernels a declared audit launches beyond it are what the
           declaration adds: none on the clean trace (a closed product queues
           nothing) -- compared as kernel lists (zkgpu_prof_kernels), not as
           times.

There is no threshold: the figures are a record.  It ends itself at
--time-limit seconds and writes what it has after every step.  GPU box.

Usage: tools/conn_cost.py [--shapes 22x12,23x2] [--audit-log-n 20] [--reps 5]
                          [--time-limit 500] out.json
"""
import argparse
import json
import os
import signal
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "zkevm-prover_amd")]

P = 0xFFFFFFFF00000001
M32 = np.uint64(0xFFFFFFFF)
KERNELS = ("k_conn_probe", "k_conn_count", "k_nz_count", "k_nz_emit", "k_conn_emit")


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4),
            "all": [round(x, 4) for x in xs]}


def mulmod(a, b):
    """a * b mod p, a a canonical uint64 array, b a canonical int (the device's folding, in numpy)"""
    b0, b1 = np.uint64(b & 0xFFFFFFFF), np.uint64(b >> 32)
    a0, a1 = a & M32, a >> np.uint64(32)
    p00 = a0 * b0
    t = a0 * b1 + (p00 >> np.uint64(32))
    u = a1 * b0 + (t & M32)
    hi = a1 * b1 + (t >> np.uint64(32)) + (u >> np.uint64(32))
    lo = (u << np.uint64(32)) | (p00 & M32)
    hh, hl = hi >> np.uint64(32), hi & M32
    t0 = lo - hh
    t0 = np.where(lo < hh, t0 - M32, t0)
    t1 = (hl << np.uint64(32)) - hl
    r = t0 + t1
    r = np.where(r < t1, r + M32, r)
    return np.where(r >= np.uint64(P), r - np.uint64(P), r)


def omega(n_bits):
    w = 7277203076849721926
    for _ in range(n_bits, 32):
        w = w * w % P
    return w


def powers(w, n_bits):
    """w^r, r < 2^n_bits, by doubling"""
    x = np.ones(1 << n_bits, np.uint64)
    for b in range(n_bits):
        m = 1 << b
        x[m:2 * m] = mulmod(x[:m], pow(w, m, P))
    return x


def wiring(n_bits, k, seed=1):
    """(a, s): k columns, column i + 1 = column i rotated by 3 + 2 i rows, the cycle closed through column 0"""
    n = 1 << n_bits
    rot = [3 + 2 * i for i in range(k - 1)]
    ks = [pow(12, i, P) for i in range(k)]
    w = omega(n_bits)
    x = powers(w, n_bits)
    a0 = np.random.default_rng(seed).integers(0, P, size=n, dtype=np.uint64)
    a = np.empty((k, n), np.uint64)
    s = np.empty((k, n), np.uint64)
    a[0] = a0
    s[0] = mulmod(x, ks[k - 1] * pow(w, -sum(rot) % n, P) % P)
    for i in range(k - 1):
        a[i + 1] = np.roll(a0, -sum(rot[:i + 1]))
        s[i + 1] = mulmod(x, ks[i] * pow(w, rot[i], P) % P)
    return a, s


def primitive(zkgpu, n_bits, k, reps, res, dump):
    n, mv = 1 << n_bits, 16
    res.update({"rows": n, "k": k, "workspace_bytes": zkgpu.conn_breaks_workspace_bytes(n, k), "cases": {}})
    a, s = wiring(n_bits, k)
    d_s = zkgpu.to_device(s.ravel())
    d_out = zkgpu.to_device(np.zeros(3 + 6 * mv, np.uint64))
    for name in ("clean", "one_cell_off"):
        if name == "one_cell_off":
            a[k - 1, n // 3] = (int(a[k - 1, n // 3]) + 1) % P
        d_a = zkgpu.to_device(a.ravel())
        wall, kern = [], {kn: [] for kn in KERNELS}
        for rep in range(reps + 1):
            zkgpu.synchronize()
            zkgpu.prof_reset()
            t0 = time.perf_counter()
            zkgpu.conn_breaks_dev(d_out, d_a, n, None, d_s, n, None, k, None, n_bits, mv)
            zkgpu.synchronize()
            t1 = time.perf_counter()
            if rep == 0:
                continue  # warm: the workspace grown
            wall.append((t1 - t0) * 1e3)
            for kn in KERNELS:
                kern[kn].append(zkgpu.prof_query(kn)[1])
        out = [int(v) for v in zkgpu.from_device(d_out)]
        res["cases"][name] = {"counts": out[:3], "first_breaks": [out[3 + 4 * e:7 + 4 * e] for e in range(2)],
                              "wall_ms": spread(wall), "kernel_ms": {kn: spread(v) for kn, v in kern.items()}}
        del d_a
        dump()


def audit(zkgpu, log_n, reps, res, dump):
    from zkgpu.stark import GpuStark
    from zkgpu.synthetic import SyntheticStark
    inst = SyntheticStark(n_bits=log_n, n_conns=1)
    cn, z = inst.conns[0], len(inst.z_ctx) - 1
    g = GpuStark(inst)
    g.witness()
    trace = g.get_cm1()
    res.update({"rows": 1 << log_n, "product": z, "cases": {}})
    row = (1 << log_n) // 3
    for fault in ("clean", "one_cell_off"):
        if fault == "one_cell_off":
            trace[row, cn["cols"][1]] = (int(trace[row, cn["cols"][1]]) + 1) % P
        g.set_cm1(trace)
        for declared in (False, True):
            if declared:
                g.conn_set(z, cn["cols"], cn["S"])
            else:
                g.conn_set(z)
            wall, lines = [], {}
            for rep in range(reps + 1):
                zkgpu.prof_reset()
                t0 = time.perf_counter()
                r = g.audit(names=True)
                t1 = time.perf_counter()
                if rep == 0:
                    continue
                wall.append((t1 - t0) * 1e3)
                for kk, v in g.timers().items():
                    lines.setdefault(kk, []).append(v)
            c = g.audit_conn(0)
            res["cases"]["%s_%s" % (fault, "declared" if declared else "undeclared")] = {
                "clean": r["clean"], "open": [e["z"] for e in r["z"]], "identities": r["identities"]["n_bad"],
                "connection": {kk: c[kk] for kk in ("ran", "n_broken", "n_foreign", "n_untargeted")},
                "breaks": c["breaks"][:2], "audit_wall_ms": spread(wall),
                "audit_ms": {kk: spread(v) for kk, v in lines.items()}, "kernels": sorted(zkgpu.prof_kernels())}
            dump()
        cs = res["cases"]
        res["kernels_added_by_the_declaration_" + fault] = sorted(
            set(cs[fault + "_declared"]["kernels"]) - set(cs[fault + "_undeclared"]["kernels"]))
        # conn_check alone: no stage program, one synchronisation
        wall = []
        for rep in range(reps + 1):
            t0 = time.perf_counter()
            g.conn_check(z)
            if rep:
                wall.append((time.perf_counter() - t0) * 1e3)
        res["conn_check_wall_ms_" + fault] = spread(wall)
        dump()
    g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="22x12,23x2")
    ap.add_argument("--audit-log-n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--time-limit", type=int, default=500)
    ap.add_argument("out")
    args = ap.parse_args()
    import zkgpu
    from zkgpu import stamp
    doc = {"what": " ".join(__doc__.split("\n\n")[0].split()), "stamps": stamp.all_stamps(), "reps": args.reps,
           "primitive": {}, "audit": {}}

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
    zkgpu.prof_enable(True)
    for shape in [s for s in args.shapes.split(",") if s]:
        n_bits, k = (int(v) for v in shape.split("x"))
        primitive(zkgpu, n_bits, k, args.reps, doc["primitive"].setdefault(shape, {}), write)
        print(shape, json.dumps(doc["primitive"][shape]), flush=True)
    if args.audit_log_n:
        audit(zkgpu, args.audit_log_n, args.reps, doc["audit"], write)
        print("audit", json.dumps(doc["audit"]), flush=True)
    zkgpu.prof_enable(False)
    signal.alarm(0)
    write()


if __name__ == "__main__":
    main()
