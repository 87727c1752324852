#!/usr/bin/env python3
"""Timing of the map partitioners (csrc/map_part.hip) and of scoring a map partition, on config 2's matrix (suitesparse_shaped,
n = m = 10^6, nnz = 13 n, K = 32) under the two row partitions of test/runbenchmarks.jl:68-69 -- the EquiSplitter split of the
adjoint and mod1.(1:m, K):

  MagneticPartitioner(seed)                      ms per call
  GreedyBottleneckPartitioner(local_model, seed) ms per call; setup / gather / walk from the profile slots, the walk's time per column,
                                                 and the same call with "greedy_lds_parts" 0 (the walk's state in global memory)
  partition_plaid(AlternatingPartitioner(LazyBisectCost(net, eps), Greedy(loc), LazyBisectCost(comm, eps)))   bin/test_table_bottleneck.jl:56
  bottleneck_value(A, Phi, net_model) of the map Phi the Greedy call returned (column gather on the device + the objective)

A call's ms is a host clock around the call, which ends in a stream sync and includes the copies of its arguments and results; the
best of --reps calls after one warm-up call.  The profile slots are read in a further call of their own.  The walk is one wave and
latency-bound: these numbers record what it costs, they claim nothing.  One JSON document, printed and written to --out."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np, torch
import cpamd
cp = cpamd.load()
import synth

SEED = 0xDEADBEEF
SLOTS = ("map_magnetic", "map_greedy_setup", "map_greedy_gather", "map_greedy_walk")


def timed(hip, f, reps):
    f()                                                       # warm: code objects, pool, upload of the pattern
    times = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter(); f(); times.append(time.perf_counter() - t0)
    hip.prof_reset(); hip.prof_enable(True)
    f()
    hip.prof_enable(False)
    pr = hip.prof_get()
    return {"ms": round(min(times) * 1e3, 3), "ms_all": [round(t * 1e3, 3) for t in times],
            "kernel_ms": {k: round(pr[k]["ms"], 3) for k in SLOTS if pr[k]["launches"]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--deg", type=int, default=13)
    ap.add_argument("--parts", type=int, default=32)
    ap.add_argument("--eps", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_map_partitioners.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_map_partitioners: no GPU; nothing is measured without one")
    dev = torch.device("cuda", 0)
    hip = cp.get_backend()
    n, K = args.n, args.parts
    m, _, colptr, rowval = synth.suitesparse_shaped_t(n, args.deg, SEED + 1, dev, nnz=args.deg * n)
    A = cp.SparseMatrixCSC(m, n, colptr.cpu().numpy(), rowval.cpu().numpy())
    del colptr, rowval
    T = cp.adjointpattern(A, backend=hip)
    net = cp.AffineConnectivityModel(0, 10, 1, 100)
    comm = cp.AffinePrimaryConnectivityModel(0, 10, 1, 0, 100)
    loc = cp.AffineSecondaryConnectivityModel(0, 10, 1, 0, 100)
    out = {"matrix": {"family": "suitesparse_shaped", "m": m, "n": n, "nnz": A.nnz, "seed": SEED + 1}, "K": K, "reps": args.reps}
    res = {}
    for key, Pi in (("Pi_spl", cp.partition_stripe(T, K, cp.EquiSplitter())), ("Pi_map", cp.MapPartition(K, np.arange(m, dtype=np.int64) % K + 1))):
        line = out[key] = {}
        line["MagneticPartitioner"] = timed(hip, lambda: cp.partition_stripe(A, K, cp.MagneticPartitioner(1), Pi, backend=hip), args.reps)

        def greedy():
            res["Phi"] = cp.partition_stripe(A, K, cp.GreedyBottleneckPartitioner(loc, seed=1), Pi, backend=hip)
        for tag, parts in (("GreedyBottleneckPartitioner", 2048), ("GreedyBottleneckPartitioner, greedy_lds_parts = 0", 0)):
            hip.set_option("greedy_lds_parts", parts)
            try:
                g = line[tag] = timed(hip, greedy, args.reps)
            finally:
                hip.set_option("greedy_lds_parts", 2048)
            g["walk_ns_per_column"] = round(g["kernel_ms"]["map_greedy_walk"] * 1e6 / n, 1)
            g["walk_ns_per_entry"] = round(g["kernel_ms"]["map_greedy_walk"] * 1e6 / A.nnz, 2)
        Phi = res["Phi"]
        v = []
        line["bottleneck_value(map Phi, net_model)"] = timed(hip, lambda: v.append(cp.bottleneck_value(A, Phi, net, backend=hip)), args.reps)
        line["bottleneck_value(map Phi, net_model)"]["value"] = int(v[-1])
        print(json.dumps({key: line}), file=sys.stderr, flush=True)
    method = cp.AlternatingPartitioner(cp.LazyBisectCostBottleneckSplitter(net, args.eps), cp.GreedyBottleneckPartitioner(loc, seed=1),
                                       cp.LazyBisectCostBottleneckSplitter(comm, args.eps))

    def plaid():
        res["plaid"] = cp.partition_plaid(A, K, method, adj_A=T, backend=hip)
    p = out["partition_plaid(AlternatingPartitioner(LazyBisectCost(net), Greedy(loc), LazyBisectCost(comm)))"] = timed(hip, plaid, args.reps)
    Pi, Phi = res["plaid"]
    p["eps"] = args.eps
    p["bottleneck_value(comm_model)"] = int(cp.bottleneck_value(A, Phi, comm, Pi, backend=hip))
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
