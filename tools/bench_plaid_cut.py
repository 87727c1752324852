#!/usr/bin/env python3
"""Timing of the total-cost DP of the plaid edge-cut models (csrc/plaid_cut.hip) on the suitesparse_shaped family (tests/synth.py,
the generator bench.py uses): partition_stripe(A, K, DynamicTotalSplitter(AffinePrimaryEdgeCutModel), Pi), Pi the EquiSplitter
partition of the rows,
  * by the prefix-min scan at n = 10^6, nnz = 10^7, K = 64 (and at n = brute_max_n, to compare),
  * by the candidate sweep (force_brute = 1) at n = brute_max_n, nnz = 10 n,
  * and, for scale, the sweep of DynamicTotalSplitter(AffinePrimaryConnectivityModel) (csrc/plaid.hip) at that size.
ms: host clock around the call, which ends in a stream sync and includes the upload of Pi and the K reads of the unravel.  The scan
is the best of --reps calls after a warm one; a sweep is one call, made after a K = 2 call on the same handle, so the code objects
are loaded and the link arrays (which only the connectivity sweep needs) are built before the clock starts.  One JSON line."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np, torch
import cpamd
cp = cpamd.load()
from bench import gen_suitesparse_shaped


def equi(m, K):
    k = np.arange(0, K + 1, dtype=np.int64)
    return cp.SplitPartition(K, k * (m // K) + np.minimum(m % K, k) + 1)              # EquiPartitioner.jl:7


def timed(f, reps, warm):
    if warm:
        f()
    best = 1e30
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter(); f(); best = min(best, time.perf_counter() - t0)
    return round(best * 1e3, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--deg", type=int, default=10)
    ap.add_argument("--K", type=int, default=64)
    ap.add_argument("--n-sweep", type=int, default=200_000, help="the library's default brute_max_n (dp_brute.hip), the largest n the candidate sweeps accept; a larger value is set as the option")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    hip = cp.get_backend()
    K = args.K
    cut = cp.AffinePrimaryEdgeCutModel(0, 10, 1, 100).marshal()
    con = cp.AffinePrimaryConnectivityModel(0, 10, 1, 0, 100).marshal()
    out = {"K": K}

    def run(n, mm, brute):
        colptr, rowval = gen_suitesparse_shaped(n, args.deg * n, 0xDEADBEEF + 2, dev)
        h = hip.csr_from_device(n, n, rowval.numel(), colptr.data_ptr(), rowval.data_ptr())
        rp, keep = cp.api._rowpart(equi(n, K))
        spl = np.zeros(K + 1, dtype=np.int64)

        def call(Kc=K):
            rc = hip.partition_dynamic(h, Kc, cp.models.CP_COMBINE_SUM, cp.models.CP_ORDER_SPLITTER, mm, rp, None, 0, 0.0, spl[:Kc + 1])
            assert rc == 0, hip.last_error()
        hip.set_option("force_brute", 1 if brute else 0)
        if brute and n > 200_000:
            hip.set_option("brute_max_n", n)
        try:
            if brute:
                call(2)
            hip.set_option("stat_reset", 1)
            ms = timed(call, 1 if brute else args.reps, not brute)
        finally:
            hip.set_option("force_brute", 0)
        res = {"n": n, "nnz": int(rowval.numel()), "ms": ms, "timing": "one call after a K = 2 call" if brute else f"best of {args.reps} after a warm call",
               "cut_scan_layers_per_call": hip.get_stat("cut_scan_layers") // (1 if brute else args.reps + 1), "spl_head": spl[:4].tolist()}
        hip.csr_destroy(h)
        print(json.dumps(res), file=sys.stderr, flush=True)
        return res
    out["primary_edge_cut_scan"] = run(args.n, cut, False)
    out["primary_edge_cut_scan_at_sweep_size"] = run(args.n_sweep, cut, False)
    out["primary_edge_cut_sweep"] = run(args.n_sweep, cut, True)
    out["primary_connectivity_sweep"] = run(args.n_sweep, con, True)
    assert out["primary_edge_cut_scan_at_sweep_size"]["spl_head"] == out["primary_edge_cut_sweep"]["spl_head"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
