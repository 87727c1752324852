#!/usr/bin/env python3
"""Timing of partition_stripe(A, K, LazyBisectCostBottleneckSplitter(comm_model, eps), Pi) with the reference's
comm_model = AffinePrimaryConnectivityModel(0, 10, 1, 0, 100) (test/runbenchmarks.jl:19, bin/test_table_bottleneck.jl:23) on the
config-2 generator (square, n = 10^6, K = 32, eps = 0.01), under Pi = partition_stripe(A', K, EquiSplitter()) and under the cyclic
MapPartition of the rows (runbenchmarks.jl:67-79).  Per Pi: time per call (median of the repeats, links cached) and per probe, next to
  (a) LazyBisectCost(AffineConnectivityModel(0, 10, 1, 100)) on the same pattern: the same stream at 4 B per entry, and
  (b) BisectCostBottleneckSplitter(comm_model, eps) with the same Pi: the only route for this model before.
Expectation, written before the first run: the primary probe reads 8 B per entry (prev and the owner) against 4, so its time per probe
is at most about twice (a)'s; (b) regroups the pattern on the host and builds a second counter in every call, so it is slower per call
by a wide margin.  Also recorded: bottleneck_value(lazy) <= (1 + eps) * bottleneck_value(BisectIndex(comm_model)).
One JSON line on stdout; --out PATH also writes it to a file (profiles/r13_lazy_primary.json is a run of this script)."""
import sys, os, time, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import numpy as np
import torch
torch.cuda.init()           # torch's HIP runtime first, then the library (as bench.py does)
from util import cp
from chainpartitioners_jl_amd import _lib, api
from bench import gen_suitesparse_shaped

out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
n = int(sys.argv[sys.argv.index("--n") + 1]) if "--n" in sys.argv else 1_000_000
hip = _lib.HipBackend()
K, eps, reps = 32, 0.01, 7
colptr, rowval = gen_suitesparse_shaped(n, 13 * n, 0xDEADBEEF + 1, torch.device("cuda", 0))
A = cp.SparseMatrixCSC(n, n, colptr.cpu().numpy(), rowval.cpu().numpy())
comm, conn = cp.AffinePrimaryConnectivityModel(0, 10, 1, 0, 100), cp.AffineConnectivityModel(0, 10, 1, 100)


def timed(call, reps):
    """(first call, sorted repeat times, result of the first call); every repeat must return the same"""
    t0 = time.perf_counter(); first_res = call(); first = time.perf_counter() - t0
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); res = call(); ts.append(time.perf_counter() - t0)
        assert res[0] == first_res[0] and np.array_equal(res[1], first_res[1])
    return first, sorted(ts), first_res


def lazy_call(mm, rp):
    def call():
        rc, spl, probes = hip.partition_lazy_bisect_cost_probes(A, K, mm, eps, rp)
        assert rc == 0, hip.last_error()
        return probes, spl
    return call


rec = {"n": n, "nnz": A.nnz, "K": K, "eps": eps, "repeats": reps,
       "expectation": "ms_per_probe(primary) <= ~2 x ms_per_probe(connectivity): 8 B per entry against 4; BisectCost(comm_model) pays a host "
                      "regrouping and a second counter build per call"}
first, ts, (probes, spl) = timed(lazy_call(conn.marshal(), None), reps)
rec["lazy_connectivity"] = {"first_call_s": first, "median_s": ts[len(ts) // 2], "min_s": ts[0], "max_s": ts[-1], "probes": probes,
                            "ms_per_probe": 1e3 * ts[len(ts) // 2] / max(probes, 1)}
k = np.arange(0, K + 1, dtype=np.int64)
for name, Pi in (("split", cp.SplitPartition(K, k * (A.m // K) + np.minimum(A.m % K, k) + 1)),
                 ("cyclic", cp.MapPartition(K, (np.arange(A.m, dtype=np.int64) % K) + 1))):
    rp, keep = api._rowpart(Pi)
    first, ts, (probes, spl) = timed(lazy_call(comm.marshal(), rp), reps)
    r = {"lazy_primary": {"first_call_s": first, "median_s": ts[len(ts) // 2], "min_s": ts[0], "max_s": ts[-1], "probes": probes,
                          "ms_per_probe": 1e3 * ts[len(ts) // 2] / max(probes, 1)}}
    r["ms_per_probe_ratio_to_connectivity"] = r["lazy_primary"]["ms_per_probe"] / rec["lazy_connectivity"]["ms_per_probe"]

    def bisect_call():
        return 0, cp.partition_stripe(A, K, cp.BisectCostBottleneckSplitter(comm, eps), Pi, backend=hip).spl
    first, ts, (_, spl_b) = timed(bisect_call, 3)
    r["bisect_cost"] = {"first_call_s": first, "median_s": ts[len(ts) // 2], "min_s": ts[0], "max_s": ts[-1]}
    r["call_time_ratio_bisect_cost_to_lazy"] = r["bisect_cost"]["median_s"] / r["lazy_primary"]["median_s"]
    spl_i = cp.partition_stripe(A, K, cp.BisectIndexBottleneckSplitter(comm), Pi, backend=hip).spl
    value = lambda s: cp.bottleneck_value(A, cp.SplitPartition(K, s), comm, Pi, backend=hip)
    r["bottleneck"] = {"lazy": value(spl), "bisect_cost": value(spl_b), "bisect_index": value(spl_i)}
    r["lazy_within_eps_of_bisect_index"] = bool(r["bottleneck"]["lazy"] <= (1 + eps) * r["bottleneck"]["bisect_index"])
    rec[name] = r
line = json.dumps(rec)
print(line, flush=True)
if out_path:
    with open(out_path, "w") as fh:
        fh.write(line + "\n")
