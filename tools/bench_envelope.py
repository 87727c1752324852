#!/usr/bin/env python3
"""Timing of the envelope cost family (csrc/envelope.hip) on  suitesparse_shaped n = 10^6  and  banded n = 5 10^6, half-bandwidth 16:
  * the builds of the reference's tree (rowenvelope) and of the sparse table, each after cp_csr_reset_cache (the arrays stay
    allocated from a first build, as in steady use);
  * 10^6 random queries env[j, j'] by the tree walk (cp_envelope_query) and 10^6 oracle evaluations on the same pairs by the sparse
    table (cp_oracle_eval) -- the comparison that says whether the table pays for its 8 B n (floor(log2 n) + 1);
  * partition_stripe(A, 32, DynamicBottleneckSplitter(AffineEnvelopeModel(0, 10, 1, 100))) by the valley search, per call and per layer;
  * the same at n = 2 10^5 by the valley search and by the candidate sweep (force_brute), the split vectors asserted equal;
  * partition_stripe(A, 32, DynamicTotalSplitter(model)) by the divide and conquer of csrc/envelope_total.hip at both sizes, and at
    n = 2 10^5 by it and by the candidate sweep, the split vectors asserted equal; the same pair at K = 8 for n = 2^7 .. 2^17 (the
    table the default of env_dc_min_n rests on);
  * BisectCostBottleneckSplitter(model, 0.01), K = 32;
  * the script pipeline PermutingPartitioner(CuthillMcKeePermuter(), DynamicBottleneckSplitter(model)), K = 32, with the bottleneck
    values with and without the reordering beside it.
ms: host clock around calls that end in a stream synchronise (they include the copies of the arguments and results), best of --reps
after one warm call; kernel_ms: the HIP-event time of the library's profile slot over the same calls, divided by the calls.  Writes
one JSON file (--out)."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np, torch
import cpamd
cp = cpamd.load()
from bench import gen_suitesparse_shaped
from bench_configs import banded_dev

MDL = cp.AffineEnvelopeModel(0, 10, 1, 100)
K = 32
ENV_DC_MIN_N = 256                                             # the library's default of env_dc_min_n (csrc/envelope_total.hip)


def clock(f):
    torch.cuda.synchronize(); t0 = time.perf_counter(); r = f(); return (time.perf_counter() - t0) * 1e3, r


def timed(hip, f, reps, slot, warm=True):
    """best host ms of `reps` calls, and the slot's kernel ms and launches per call"""
    if warm:
        f()
    hip.prof_reset(); hip.prof_enable(True)
    best, r = 1e30, None
    for _ in range(reps):
        t, r = clock(f)
        best = min(best, t)
    p = hip.prof_get()[slot]
    hip.prof_enable(False)
    return {"ms": round(best, 3), "kernel_ms": round(p["ms"] / reps, 4), "launches": p["launches"] // reps}, r


def host_matrix(n, colptr, rowval):
    return cp.SparseMatrixCSC(n, n, colptr.cpu().numpy(), rowval.cpu().numpy())


def structure(hip, A, reps, nq):
    out = {"table_bytes": 8 * A.n * int(np.floor(np.log2(A.n)) + 1), "tree_bytes": 8 * ((2 << (A.n - 1).bit_length()) - 1)}
    env = cp.rowenvelope(A, backend=hip)

    def build_tree():
        hip.reset_cache(A); return env.query([1], [A.n + 1])
    one = (np.ones(1, dtype=np.int64), np.full(1, A.n + 1, dtype=np.int64), np.zeros(1, dtype=np.int64))
    mm = MDL.marshal()

    def build_table():
        hip.reset_cache(A); return hip.oracle_eval(A, mm, None, 3, one[0], one[1], None, one[2])
    out["build_tree"], _ = timed(hip, build_tree, reps, "env_build")
    out["build_table"], _ = timed(hip, build_table, reps, "env_build")
    rng = np.random.default_rng(5)
    j = rng.integers(1, A.n + 2, nq).astype(np.int64)
    jp = (j + (rng.random(nq) * (A.n + 2 - j)).astype(np.int64)).astype(np.int64)
    res = np.zeros(nq, dtype=np.int64)
    out["queries"] = nq
    out["query_tree_walk"], (lo, hi) = timed(hip, lambda: env.query(j, jp), reps, "count_query")
    out["oracle_sparse_table"], _ = timed(hip, lambda: hip.oracle_eval(A, mm, None, 3, j, jp, None, res), reps, "count_query")
    span = np.maximum(hi - lo, 0)
    pos = np.asarray(A.colptr, dtype=np.int64)
    assert np.array_equal(res, (jp - j) * 10 + (pos[jp - 1] - pos[j - 1]) + span * 100)      # the two structures hold the same integers
    return out


def partitioners(hip, A, reps):
    out = {}
    dyn = cp.DynamicBottleneckSplitter(MDL)
    hip.set_option("stat_reset", 0)
    out["dynamic_bottleneck_K32"], Phi = timed(hip, lambda: cp.partition_stripe(A, K, dyn, backend=hip), reps, "env_valley")
    r = out["dynamic_bottleneck_K32"]
    r["kernel_ms_per_layer"] = round(r["kernel_ms"] / max(r["launches"], 1), 4)
    r["env_valley_layers_per_call"] = hip.get_stat("env_valley_layers") // (reps + 1)
    r["bottleneck_value"] = int(cp.bottleneck_value(A, Phi, MDL, backend=hip))
    out["bisect_cost_eps0.01_K32"], Phi2 = timed(hip, lambda: cp.partition_stripe(A, K, cp.BisectCostBottleneckSplitter(MDL, 0.01), backend=hip), reps, "bisect_probe")
    out["bisect_cost_eps0.01_K32"]["bottleneck_value"] = int(cp.bottleneck_value(A, Phi2, MDL, backend=hip))
    pipe = cp.PermutingPartitioner(cp.CuthillMcKeePermuter(), dyn)
    out["rcm_pipeline_K32"], Phi3 = timed(hip, lambda: cp.partition_stripe(A, K, pipe, backend=hip), 1, "env_valley")
    out["rcm_pipeline_K32"]["bottleneck_value"] = int(cp.bottleneck_value(A, Phi3, MDL, backend=hip))
    return out


def valley_against_sweep(hip, A, reps):
    dyn = cp.DynamicBottleneckSplitter(MDL)
    out = {"n": A.n, "nnz": A.nnz}
    out["valley"], a = timed(hip, lambda: cp.partition_stripe(A, K, dyn, backend=hip), reps, "env_valley")
    hip.set_option("force_brute", 1)
    try:
        cp.partition_stripe(A, 2, dyn, backend=hip)             # (code objects)
        out["sweep"], b = timed(hip, lambda: cp.partition_stripe(A, K, dyn, backend=hip), 1, "env_sweep", warm=False)
    finally:
        hip.set_option("force_brute", 0)
    assert np.array_equal(a.spl, b.spl), "the valley search and the candidate sweep disagree"
    out["same_split_vector"] = True
    return out


def total_dp(hip, A, reps):
    """partition_stripe(A, 32, DynamicTotalSplitter(model)) by the divide and conquer of envelope_total.hip (default options)"""
    tot = cp.DynamicTotalSplitter(MDL)
    hip.set_option("stat_reset", 0)
    r, Phi = timed(hip, lambda: cp.partition_stripe(A, K, tot, backend=hip), reps, "env_dc")
    r["kernel_ms_per_layer"] = round(r["kernel_ms"] / max(r["launches"], 1), 4)
    r["env_dc_layers_per_call"] = hip.get_stat("env_dc_layers") // (reps + 1)
    r["total_value"] = int(cp.total_value(A, Phi, MDL, backend=hip))
    return {"dynamic_total_K32": r}


def total_both_paths(hip, A, k, reps):
    """the total DP at K = k by the divide and conquer (env_dc_min_n = 0) and by the candidate sweep (force_brute), one after the other"""
    tot = cp.DynamicTotalSplitter(MDL)
    out = {"n": A.n, "nnz": A.nnz, "K": k}
    hip.set_option("env_dc_min_n", 0)
    try:
        out["divide_and_conquer"], a = timed(hip, lambda: cp.partition_stripe(A, k, tot, backend=hip), reps, "env_dc")
        hip.set_option("force_brute", 1)
        out["sweep"], b = timed(hip, lambda: cp.partition_stripe(A, k, tot, backend=hip), 1 if A.n > 100_000 else reps, "env_sweep")
    finally:
        hip.set_option("force_brute", 0)
        hip.set_option("env_dc_min_n", ENV_DC_MIN_N)
    assert np.array_equal(a.spl, b.spl), "the divide and conquer and the candidate sweep disagree"
    out["same_split_vector"] = True
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-shaped", type=int, default=1_000_000)
    ap.add_argument("--deg", type=int, default=10)
    ap.add_argument("--n-banded", type=int, default=5_000_000)
    ap.add_argument("--n-sweep", type=int, default=200_000)
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip", default="", help="comma list of shaped, banded, sweep (families and the n-sweep comparisons); structure, bottleneck, total, "
                                               "crossover (sections)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_envelope.json"))
    args = ap.parse_args()
    skip = set(args.skip.split(","))
    dev = torch.device("cuda", 0)
    hip = cp.get_backend()
    out = {"device": torch.cuda.get_device_name(0), "model": "AffineEnvelopeModel(0, 10, 1, 100)", "K": K, "reps": args.reps,
           "method": "host clock around synchronising calls, best of reps after a warm call; kernel_ms: HIP events of the profile slot per call",
           "note": "one run of this script: single measurements, the spread between runs was not measured"}
    warm = host_matrix(3000, *banded_dev(3000, 4, 0.5, 7, dev))    # code objects
    partitioners(hip, warm, 1); structure(hip, warm, 1, 1000)

    def family(tag, A):
        res = {"n": A.n, "nnz": A.nnz}
        hip.csr(A)
        for name, section in (("structure", lambda: structure(hip, A, args.reps, args.queries)), ("bottleneck", lambda: partitioners(hip, A, args.reps)),
                              ("total", lambda: total_dp(hip, A, args.reps))):
            if name not in skip:
                res.update(section())
                print(json.dumps({tag: res}), file=sys.stderr, flush=True)
        return res
    if "shaped" not in skip:
        n = args.n_shaped
        out["suitesparse_shaped"] = family("suitesparse_shaped", host_matrix(n, *gen_suitesparse_shaped(n, args.deg * n, 0xDEADBEEF + 2, dev)))
    if "banded" not in skip:
        n = args.n_banded
        out["banded"] = family("banded", host_matrix(n, *banded_dev(n, 16, 0.5, 0xDEADBEEF + 4, dev)))
    if "sweep" not in skip:
        n = args.n_sweep
        A = host_matrix(n, *gen_suitesparse_shaped(n, args.deg * n, 0xDEADBEEF + 2, dev))
        if "bottleneck" not in skip:
            out["valley_against_sweep"] = valley_against_sweep(hip, A, args.reps)
        if "total" not in skip:
            out["total_against_sweep"] = total_both_paths(hip, A, K, args.reps)
    if "crossover" not in skip:                                # what the default of env_dc_min_n rests on
        out["total_crossover_K8"] = [total_both_paths(hip, host_matrix(1 << lg, *gen_suitesparse_shaped(1 << lg, args.deg << lg, 0xDEADBEEF + 2, dev)), 8, args.reps)
                                     for lg in range(7, 18)]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
