#!/usr/bin/env python3
"""Timing of the symmetric lazy splitter: partition_stripe(A, K, LazyBisectCostBottleneckSplitter(sym_model, eps)) with the reference's
sym_model = AffineMonotonizedSymmetricConnectivityModel(0, 0, 1, 100, 90) (bin/test_table_bottleneck.jl:22) on the config-2 generator
(square, n = 10^6, K = 32, eps = 0.01), and in the same run the Connectivity lazy splitter with (0, 10, 1, 100).  One JSON line:
both times (median of the repeats, links and counters cached), the probe counts and the time per probe.  The symmetric probe streams
nnz + (missing diagonal entries) link entries where the Connectivity probe streams nnz."""
import sys, os, time, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import numpy as np
import torch
torch.cuda.init()           # torch's HIP runtime first, then the library (as bench.py does)
from util import cp
from chainpartitioners_jl_amd import _lib
from bench import gen_suitesparse_shaped

hip = _lib.HipBackend()
n, K, eps, reps = 1_000_000, 32, 0.01, 7
colptr, rowval = gen_suitesparse_shaped(n, 13 * n, 0xDEADBEEF + 1, torch.device("cuda", 0))
A = cp.SparseMatrixCSC(n, n, colptr.cpu().numpy(), rowval.cpu().numpy())
cols = np.repeat(np.arange(1, n + 1, dtype=np.int64), np.diff(A.colptr))
missing = n - int(np.count_nonzero(A.rowval == cols))
rec = {"n": n, "nnz": A.nnz, "K": K, "eps": eps, "missing_diagonals": missing, "stream_ratio_expected": (A.nnz + missing) / A.nnz}
for name, mdl in (("sym", cp.AffineMonotonizedSymmetricConnectivityModel(0, 0, 1, 100, 90)), ("conn", cp.AffineConnectivityModel(0, 10, 1, 100))):
    mm = mdl.marshal()
    t0 = time.perf_counter(); rc, spl, probes = hip.partition_lazy_bisect_cost_probes(A, K, mm, eps); first = time.perf_counter() - t0
    assert rc == 0, hip.last_error()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); rc, spl2, p2 = hip.partition_lazy_bisect_cost_probes(A, K, mm, eps); ts.append(time.perf_counter() - t0)
        assert rc == 0 and p2 == probes and np.array_equal(spl, spl2)
    ts.sort()
    rec[name] = {"first_call_s": first, "median_s": ts[len(ts) // 2], "min_s": ts[0], "max_s": ts[-1], "probes": probes,
                 "ms_per_probe": 1e3 * ts[len(ts) // 2] / max(probes, 1), "bottleneck": cp.bottleneck_value(A, cp.SplitPartition(K, spl), mdl, backend=hip)}
rec["ms_per_probe_ratio"] = rec["sym"]["ms_per_probe"] / rec["conn"]["ms_per_probe"]
print(json.dumps(rec), flush=True)
