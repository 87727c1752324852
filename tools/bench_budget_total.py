#!/usr/bin/env python3
"""Timing of partition_stripe(A, K, DynamicTotalSplitter(ConstrainedCost(AffineConnectivityModel(0,0,0,1), AffineWorkModel(0,0,1),
ceil(1.3 nnz / K)))) -- minimum communication volume under a pin budget per part -- on the bench-shaped pattern (nnz = deg * n):
the two-staircase divide and conquer of csrc/dp_total_budget.hip with its dp_budget time and launches per layer (best of --reps after a
warm call, host clock), both paths at the small sizes of --cross-ns (cp_set_option("force_brute", 1): the one-wave literal kernel), the
largest of which is the baseline.  Writes the JSON to --out and prints it as one line."""
import argparse, json, math, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np, torch
import cpamd
cp = cpamd.load()
from bench import gen_suitesparse_shaped

MODEL = cp.AffineConnectivityModel(0, 0, 0, 1)
PINS = cp.AffineWorkModel(0, 0, 1)


def matrix(n, deg, dev):
    colptr, rowval = gen_suitesparse_shaped(n, deg * n, 0xDEADBEEF + 2, dev)
    return cp.SparseMatrixCSC(n, n, colptr.cpu().numpy(), rowval.cpu().numpy())


def method(A, K):
    return cp.DynamicTotalSplitter(cp.ConstrainedCost(MODEL, PINS, math.ceil(1.3 * A.nnz / K)))


def best_of(hip, A, K, reps):
    best, P = None, None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        P = cp.partition_stripe(A, K, method(A, K), backend=hip)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="100000,1000000")
    ap.add_argument("--cross-ns", default="500,1500,6000")
    ap.add_argument("--deg", type=int, default=10)
    ap.add_argument("--K", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_budget_total.json"))
    ap.add_argument("--opt", action="append", default=[])
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    hip = cp.get_backend()
    for kv in args.opt:
        k, v = kv.split("="); assert hip.set_option(k, int(v)) == 0
    K = args.K
    out = {"method": "DynamicTotalSplitter(ConstrainedCost(AffineConnectivityModel(0,0,0,1), AffineWorkModel(0,0,1), ceil(1.3 nnz / K)))",
           "deg": args.deg, "K": K, "reps": args.reps, "budget_total": [], "both_paths": []}
    for n in [int(x) for x in args.ns.split(",") if x]:
        A = matrix(n, args.deg, dev)
        cp.partition_stripe(A, K, method(A, K), backend=hip)            # warm: counters, link arrays, pool
        dt, P = best_of(hip, A, K, args.reps)
        hip.set_option("stat_reset", 0)
        hip.prof_reset(); hip.prof_enable(True)
        cp.partition_stripe(A, K, method(A, K), backend=hip)
        hip.prof_enable(False)
        pr, layers = hip.prof_get()["dp_budget"], hip.get_stat("budget_layers")
        spl, pos = np.asarray(P.spl, dtype=np.int64), np.asarray(A.colptr, dtype=np.int64)
        pins = (pos[spl[1:] - 1] - pos[spl[:-1] - 1]).max()
        out["budget_total"].append({"n": n, "nnz": int(A.nnz), "budget": math.ceil(1.3 * A.nnz / K), "seconds": round(dt, 4),
                                    "dp_budget_ms_profiled": round(pr["ms"], 2), "dp_budget_launches": pr["launches"], "layers": layers,
                                    "launches_per_layer": round(pr["launches"] / max(layers, 1), 1), "max_pins_per_part": int(pins),
                                    "total_value": int(cp.total_value(A, P, MODEL, backend=hip))})
        print(json.dumps(out["budget_total"][-1]), file=sys.stderr, flush=True)
        del A
    for n in [int(x) for x in args.cross_ns.split(",") if x]:
        A = matrix(n, args.deg, dev)
        cp.partition_stripe(A, K, method(A, K), backend=hip)
        t_new, P1 = best_of(hip, A, K, args.reps)
        hip.set_option("force_brute", 1)
        try:
            t_one, P0 = best_of(hip, A, K, 1 if n > 2000 else args.reps)
        finally:
            hip.set_option("force_brute", 0)
        assert P0 == P1
        out["both_paths"].append({"n": n, "nnz": int(A.nnz), "seconds": round(t_new, 5), "force_brute_seconds": round(t_one, 5)})
        print(json.dumps(out["both_paths"][-1]), file=sys.stderr, flush=True)
    if out["both_paths"]:
        out["baseline_force_brute"] = out["both_paths"][-1]
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
