#!/usr/bin/env python3
"""Timing of partition_stripe(A, K, DynamicTotalSplitter(f), Pi) for the plaid connectivity pair on the exact paths of
csrc/plaid_total.hip: f = AffinePrimaryConnectivityModel(0, 10, 1, 0, 100) on A and its secondary twin on adjointpattern(A); a banded
pattern and a bench-shaped one with nnz = 10 n; Pi in K bands along the diagonal with one row in ten strayed (the secondary model
takes the bands as a SplitPartition); K = 16; best of --reps after a warm call (host clock).

  --cross-ns   the new path ("plaid_total_min_n" = "plaid_scan_min_n" = 0) against the candidate sweep ("force_brute" 1), the same split
               vector asserted: the crossover table of DESIGN 5d and the run at n = 200 000
  --ns         the new path at the default options with the dp_plaid_total time and its launches per layer

Expectation written down before the first run: the primary within about twice sym_total's kind-10 time at the same n (0.28 s at
n = 200 000: the same engine, two rank queries per cell plus the Lk load); the secondary near the edge-cut scan's 12 ms at n = 10^6,
K = 64.  Single measurements; no test asserts a time.  The JSON is rewritten to --out after every measurement and printed as one line
at the end."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np, torch
import cpamd
cp = cpamd.load()
from util import suitesparse_shaped, banded

PRM = (0, 10, 1, 0, 100)
SP = cp.DynamicTotalSplitter


def matrix(kind, n):
    return banded(n, 5, 0.9, 7) if kind == "banded" else suitesparse_shaped(n, 10, 3, nnz=10 * n)


def bands(m, K, stray, seed=2):
    own = 1 + (np.arange(m, dtype=np.int64) * K) // m
    if stray:
        rng = np.random.default_rng(seed)
        s = rng.random(m) < stray
        own[s] = rng.integers(1, K + 1, int(s.sum()))
        return cp.MapPartition(K, own)
    return cp.SplitPartition(K, np.linspace(1, m + 1, K + 1).astype(np.int64))


def best_of(hip, A, K, mdl, Pi, reps):
    best, P = None, None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        P = cp.partition_stripe(A, K, SP(mdl), Pi, backend=hip)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, P


def profiled(hip, A, K, mdl, Pi):
    hip.set_option("stat_reset", 0)
    hip.prof_reset(); hip.prof_enable(True)
    cp.partition_stripe(A, K, SP(mdl), Pi, backend=hip)
    hip.prof_enable(False)
    pr = hip.prof_get()["dp_plaid_total"]
    layers = hip.get_stat("plaid_total_layers") + hip.get_stat("plaid_scan_layers")
    return {"dp_plaid_total_ms_profiled": round(pr["ms"], 2), "launches": pr["launches"], "layers": layers,
            "launches_per_layer": round(pr["launches"] / max(layers, 1), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="1000000")
    ap.add_argument("--cross-ns", default="1024,2048,4096,8192,10240,16384,200000")
    ap.add_argument("--patterns", default="banded,shaped")
    ap.add_argument("--sides", default="primary,secondary")
    ap.add_argument("--K", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_plaid_total.json"))
    args = ap.parse_args()
    hip = cp.get_backend()
    K = args.K
    out = {"method": f"DynamicTotalSplitter(f), f: primary / secondary connectivity {PRM}", "K": K, "reps": args.reps,
           "expectation": "primary within about 2x sym_total's kind-10 time (0.28 s at n = 200000); secondary near the cut scan's 12 ms at n = 1e6, K = 64",
           "against_the_sweep": [], "at_the_defaults": []}

    def record(section, row):
        out[section].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")

    def sides(A):
        for side in [s for s in args.sides.split(",") if s]:
            if side == "primary":
                yield side, A, cp.AffinePrimaryConnectivityModel(*PRM), bands(A.m, K, 0.1)
            else:
                T = cp.adjointpattern(A, backend=hip)
                yield side, T, cp.AffineSecondaryConnectivityModel(*PRM), bands(T.m, K, 0)

    pats = [p for p in args.patterns.split(",") if p]
    for n in [int(x) for x in args.ns.split(",") if x]:
        for pat in pats:
            for side, X, mdl, Pi in sides(matrix(pat, n)):
                cp.partition_stripe(X, K, SP(mdl), Pi, backend=hip)
                dt, P = best_of(hip, X, K, mdl, Pi, args.reps)
                row = dict(pattern=pat, side=side, n=n, nnz=int(X.nnz), seconds=round(dt, 4), **profiled(hip, X, K, mdl, Pi))
                row["total_value"] = int(cp.total_value(X, P, mdl, Pi, backend=hip))
                record("at_the_defaults", row)
    for n in [int(x) for x in args.cross_ns.split(",") if x]:
        for pat in pats:
            for side, X, mdl, Pi in sides(matrix(pat, n)):
                for name in ("plaid_total_min_n", "plaid_scan_min_n"):
                    hip.set_option(name, 0)
                cp.partition_stripe(X, K, SP(mdl), Pi, backend=hip)          # warm: counters, link arrays, pool
                t_new, P1 = best_of(hip, X, K, mdl, Pi, args.reps)
                hip.set_option("force_brute", 1)
                try:
                    t_old, P0 = best_of(hip, X, K, mdl, Pi, 1 if n > 20000 else args.reps)
                finally:
                    hip.set_option("force_brute", 0)
                assert P0 == P1, (pat, n, side)
                record("against_the_sweep", {"pattern": pat, "side": side, "n": n, "nnz": int(X.nnz), "seconds": round(t_new, 5),
                                             "force_brute_seconds": round(t_old, 5), "parts_used": len(set(P1.spl.tolist())) - 1})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
