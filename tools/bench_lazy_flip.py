#!/usr/bin/env python3
"""Timing of the row sweep of the reference's lazy alternating partitioner (bin/test_table_bottleneck.jl:48):
partition_stripe(T, K, LazyFlipBisectCostBottleneckSplitter(loc_model, eps), Phi) with loc_model =
AffineSecondaryConnectivityModel(0, 10, 1, 0, 100), T = adjointpattern(A) and Phi = partition_stripe(A, K, LazyBisectCost(net_model,
eps)), on the config-2 generator (square, n = 10^6, K = 32, eps = 0.01).  Time per call (median of the repeats, links cached) and per
probe, next to
  (a) FlipBisectCostBottleneckSplitter(loc_model, eps) on the same (T, Phi): the only route for the row sweep before, and
  (b) LazyBisectCost(net_model, eps) on A, per probe: the connectivity stream at 4 B per entry.
Expectation, written before the first run: the secondary probe streams one 4-byte array (e2) like (b), so its time per probe is about
(b)'s, 4.3 ms in profiles/r13_lazy_primary.json; a call adds the gather of e2 (row, owner, column of every entry) and an upload of the
owner array.  Also recorded: bottleneck_value(lazy flip) <= (1 + eps) * bottleneck_value(FlipBisectIndex(loc_model)).
One JSON line on stdout; --out PATH also writes it to a file (profiles/r14_lazy_flip.json is a run of this script)."""
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
net, loc = cp.AffineConnectivityModel(0, 10, 1, 100), cp.AffineSecondaryConnectivityModel(0, 10, 1, 0, 100)


def timed(call, reps):
    """(first call, sorted repeat times, result of the first call); every repeat must return the same"""
    t0 = time.perf_counter(); first_res = call(); first = time.perf_counter() - t0
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); res = call(); ts.append(time.perf_counter() - t0)
        assert res[0] == first_res[0] and np.array_equal(res[1], first_res[1])
    return first, sorted(ts), first_res


def stats(first, ts, probes=None):
    r = {"first_call_s": first, "median_s": ts[len(ts) // 2], "min_s": ts[0], "max_s": ts[-1]}
    if probes is not None:
        r.update(probes=probes, ms_per_probe=1e3 * ts[len(ts) // 2] / max(probes, 1))
    return r


def lazy_net():
    rc, spl, probes = hip.partition_lazy_bisect_cost_probes(A, K, net.marshal(), eps)
    assert rc == 0, hip.last_error()
    return probes, spl


rec = {"n": n, "nnz": A.nnz, "K": K, "eps": eps, "repeats": reps,
       "expectation": "ms_per_probe(lazy flip, secondary) ~ ms_per_probe(lazy connectivity) ~ 4.3 ms: both stream 4 B per entry; "
                      "FlipBisectCost(loc_model) pays a host regrouping, a second matrix and a second counter per call"}
first, ts, (probes, phi) = timed(lazy_net, reps)
rec["lazy_connectivity"] = stats(first, ts, probes)
Phi = cp.SplitPartition(K, phi)
T = cp.adjointpattern(A, backend=hip)
rp, keep = api._rowpart(Phi)


def lazy_flip():
    rc, spl, probes = hip.partition_lazy_flip_bisect_cost_probes(T, K, loc.marshal(), eps, rp)
    assert rc == 0, hip.last_error()
    return probes, spl


def flip_bisect():
    return 0, cp.partition_stripe(T, K, cp.FlipBisectCostBottleneckSplitter(loc, eps), Phi, backend=hip).spl


first, ts, (probes, spl) = timed(lazy_flip, reps)
rec["lazy_flip_secondary"] = stats(first, ts, probes)
rec["ms_per_probe_ratio_to_connectivity"] = rec["lazy_flip_secondary"]["ms_per_probe"] / rec["lazy_connectivity"]["ms_per_probe"]
first, ts, (_, spl_b) = timed(flip_bisect, 3)
rec["flip_bisect_cost"] = stats(first, ts)
rec["call_time_ratio_flip_bisect_cost_to_lazy_flip"] = rec["flip_bisect_cost"]["median_s"] / rec["lazy_flip_secondary"]["median_s"]
spl_i = cp.partition_stripe(T, K, cp.FlipBisectIndexBottleneckSplitter(loc), Phi, backend=hip).spl
value = lambda s: cp.bottleneck_value(T, cp.SplitPartition(K, s), loc, Phi, backend=hip)
rec["bottleneck"] = {"lazy_flip": value(spl), "flip_bisect_cost": value(spl_b), "flip_bisect_index": value(spl_i)}
rec["lazy_flip_within_eps_of_flip_bisect_index"] = bool(rec["bottleneck"]["lazy_flip"] <= (1 + eps) * rec["bottleneck"]["flip_bisect_index"])
line = json.dumps(rec)
print(line, flush=True)
if out_path:
    with open(out_path, "w") as fh:
        fh.write(line + "\n")
