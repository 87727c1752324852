#!/usr/bin/env python3
"""Timing of partition_stripe(A, K, DynamicTotalSplitter(f)) for the three symmetric cost models on the divide and conquer of
csrc/sym_total.hip: a symmetrised bench-shaped pattern (nnz ~ deg * n) and a banded one, K = 16, best of --reps after a warm call
(host clock).  At the sizes of --cross-ns the new path against the candidate sweep (cp_set_option("force_brute", 1)), the same split
vector asserted; at the sizes of --ns the batched launch form against the per-rectangle form ("sym_total_batch" 1 / 0) with the
dp_sym_total time and launches per layer.  The JSON is rewritten to --out after every measurement and printed as one line at the end."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np, torch
import cpamd
cp = cpamd.load()
from util import suitesparse_shaped, banded

MODELS = {"sym_conn": cp.AffineSymmetricConnectivityModel(0, 0, 0, 1, 2), "mono_sym": cp.AffineMonotonizedSymmetricConnectivityModel(0, 0, 1, 100, 2),
          "sym_edge_cut": cp.AffineSymmetricEdgeCutModel(0, 0, 0, 1)}


def matrix(kind, n, deg):
    if kind == "banded":
        return banded(n, deg // 2, 1.0, 7)
    B = suitesparse_shaped(n, deg // 2, 3, nnz=(deg // 2) * n)         # united with its transpose: about deg * n nonzeros
    cols = np.repeat(np.arange(n, dtype=np.int64), np.diff(B.colptr))
    rows = np.asarray(B.rowval, dtype=np.int64) - 1
    key = np.unique(np.concatenate([cols * n + rows, rows * n + cols]))
    colptr = np.concatenate([[1], 1 + np.cumsum(np.bincount(key // n, minlength=n))]).astype(np.int64)
    return cp.SparseMatrixCSC(n, n, colptr, key % n + 1)


def best_of(hip, A, K, mdl, reps):
    best, P = None, None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        P = cp.partition_stripe(A, K, cp.DynamicTotalSplitter(mdl), backend=hip)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, P


def profiled(hip, A, K, mdl):
    hip.set_option("stat_reset", 0)
    hip.prof_reset(); hip.prof_enable(True)
    cp.partition_stripe(A, K, cp.DynamicTotalSplitter(mdl), backend=hip)
    hip.prof_enable(False)
    pr, layers = hip.prof_get()["dp_sym_total"], hip.get_stat("sym_total_layers")
    return {"dp_sym_total_ms_profiled": round(pr["ms"], 2), "launches": pr["launches"], "layers": layers,
            "launches_per_layer": round(pr["launches"] / max(layers, 1), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="1000000")
    ap.add_argument("--cross-ns", default="200000")
    ap.add_argument("--patterns", default="shaped,banded")
    ap.add_argument("--models", default=",".join(MODELS))
    ap.add_argument("--deg", type=int, default=10)
    ap.add_argument("--K", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_sym_total.json"))
    ap.add_argument("--opt", action="append", default=[])
    args = ap.parse_args()
    hip = cp.get_backend()
    for kv in args.opt:
        k, v = kv.split("="); assert hip.set_option(k, int(v)) == 0
    K = args.K
    out = {"method": "DynamicTotalSplitter(f), f: " + ", ".join(f"{k} {m._params()}" for k, m in MODELS.items()), "deg": args.deg, "K": K,
           "reps": args.reps, "opts": args.opt, "against_the_sweep": [], "batch_against_per_rectangle": []}

    def record(section, row):
        out[section].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")

    pats, names = [p for p in args.patterns.split(",") if p], [m for m in args.models.split(",") if m]
    for n in [int(x) for x in args.cross_ns.split(",") if x]:
        hip.set_option("brute_max_n", max(n, 200000))
        for pat in pats:
            A = matrix(pat, n, args.deg)
            for name in names:
                mdl = MODELS[name]
                cp.partition_stripe(A, K, cp.DynamicTotalSplitter(mdl), backend=hip)      # warm: counters, link arrays, pool
                t_new, P1 = best_of(hip, A, K, mdl, args.reps)
                hip.set_option("force_brute", 1)
                try:
                    t_old, P0 = best_of(hip, A, K, mdl, 1 if n > 20000 else args.reps)
                finally:
                    hip.set_option("force_brute", 0)
                assert P0 == P1, (pat, n, name)
                record("against_the_sweep", {"pattern": pat, "n": n, "nnz": int(A.nnz), "model": name, "seconds": round(t_new, 5),
                                             "force_brute_seconds": round(t_old, 5), "parts_used": len(set(P1.spl.tolist())) - 1})
            del A
    for n in [int(x) for x in args.ns.split(",") if x]:
        for pat in pats:
            A = matrix(pat, n, args.deg)
            for name in names:
                mdl = MODELS[name]
                row = {"pattern": pat, "n": n, "nnz": int(A.nnz), "model": name}
                parts = []
                for batch in (1, 0):
                    hip.set_option("sym_total_batch", batch)
                    try:
                        cp.partition_stripe(A, K, cp.DynamicTotalSplitter(mdl), backend=hip)
                        dt, P = best_of(hip, A, K, mdl, args.reps)
                        row["batch_%d" % batch] = dict(seconds=round(dt, 4), **profiled(hip, A, K, mdl))
                        parts.append(P)
                    finally:
                        hip.set_option("sym_total_batch", 1)
                assert parts[0] == parts[1], (pat, n, name)
                row["total_value"] = int(cp.total_value(A, parts[0], mdl, backend=hip))
                record("batch_against_per_rectangle", row)
            del A
    print(json.dumps(out))


if __name__ == "__main__":
    main()
