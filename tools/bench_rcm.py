#!/usr/bin/env python3
"""Timing of the reordering layer (csrc/rcm.hip): permute_plaid(A, CuthillMcKeePermuter()), permute(A, sigma, tau) and the pipeline of
the reference's bottleneck script (bin/test_table_bottleneck.jl:49),
    PermutingPartitioner(CuthillMcKeePermuter(), SymmetricPartitioner(LazyBisectCostBottleneckSplitter(sym_model, eps))),  K = 16,
on  suitesparse_shaped n = 10^6 (not symmetric: the bipartite walk over 2 n vertices), a symmetrised copy of it (the symmetric walk)
and  banded n = 5 10^6, half-bandwidth 16 (about n / 16 BFS levels of a few dozen vertices: the case the one-workgroup walker is for).

permute_plaid runs once per value of the option "rcm_narrow" (--narrow; 0 = every level by grid kernels, a large value = the walker
whenever the level fits), with the counters of cp_rcm beside each time; every value must give the same permutations.  Times are host
clock around calls that end in a stream synchronise, after one warm call at a small size (code objects) and with the pattern and its
adjoint resident; they include the copies of the results to the host.  For scale, the host key formulation of tests/rcm_model.py at
n = 10^5 on the banded family, labelled as Python.  Writes one JSON file (--out)."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np, torch
import cpamd
cp = cpamd.load()
from bench import gen_suitesparse_shaped
from bench_configs import banded_dev

DEFAULT_NARROW = 256                                              # the library's default of the option (csrc/rcm.hip)
RCM = cp.CuthillMcKeePermuter()
SYM_MODEL = cp.AffineMonotonizedSymmetricConnectivityModel(0, 0, 1, 100, 90)      # bin/test_table_bottleneck.jl:22
PIPELINE = cp.PermutingPartitioner(RCM, cp.SymmetricPartitioner(cp.LazyBisectCostBottleneckSplitter(SYM_MODEL, 0.01)))


def clock(f):
    torch.cuda.synchronize(); t0 = time.perf_counter(); r = f(); return time.perf_counter() - t0, r


def symmetrised(colptr, rowval, n):
    cols = torch.repeat_interleave(torch.arange(n, device=colptr.device), colptr[1:] - colptr[:-1])
    rows = rowval - 1
    key = torch.unique(torch.cat([cols * n + rows, rows * n + cols]))
    cols = key // n
    cp_ = torch.cat([torch.ones(1, dtype=torch.int64, device=colptr.device), 1 + torch.cumsum(torch.bincount(cols, minlength=n), 0)])
    return cp_.contiguous(), ((key % n) + 1).contiguous()


def host_matrix(n, colptr, rowval):
    return cp.SparseMatrixCSC(n, n, colptr.cpu().numpy(), rowval.cpu().numpy())


def measure(hip, tag, A, narrows, reps, off_reps):
    out = {"family": tag, "m": A.m, "n": A.n, "nnz": A.nnz}
    hip.csr(A)                                                     # resident before anything is timed
    out["adjointpattern_ms"], T = clock(lambda: cp.adjointpattern(A, backend=hip))
    out["adjointpattern_ms"] = round(out["adjointpattern_ms"] * 1e3, 2)
    first = None
    out["permute_plaid"] = {}
    for nv in narrows:
        hip.set_option("rcm_narrow", nv)
        times = []
        for _ in range(off_reps if nv == 0 else reps):
            t, (s, t_) = clock(lambda: cp.permute_plaid(A, RCM, adj_A=T, backend=hip))
            times.append(t)
        stats = dict(hip.last_rcm_stats)
        if first is None:
            first = (s, t_)
        same = bool(np.array_equal(s.prm, first[0].prm) and np.array_equal(t_.prm, first[1].prm))
        out["permute_plaid"][f"rcm_narrow={nv}"] = {"ms": [round(x * 1e3, 2) for x in times], "same_permutation": same, **stats}
        print(json.dumps({tag: {f"rcm_narrow={nv}": out["permute_plaid"][f"rcm_narrow={nv}"]}}), file=sys.stderr, flush=True)
    hip.set_option("rcm_narrow", DEFAULT_NARROW)                  # permute and the pipeline run at the library's default
    s, t_ = first
    times = [clock(lambda: cp.permute(A, s, t_, backend=hip))[0] for _ in range(reps)]
    out["permute_ms"] = [round(x * 1e3, 2) for x in times]
    times = []
    for _ in range(reps):
        t, (Pi, Phi) = clock(lambda: cp.partition_plaid(A, 16, PIPELINE, adj_A=T, backend=hip))
        times.append(t)
    asg = cp.to_map(Phi).asg
    out["pipeline_K16_ms"] = [round(x * 1e3, 2) for x in times]
    out["pipeline_covers_once"] = bool(np.array_equal(np.sort(Phi.prm), np.arange(1, A.n + 1)) and asg.min() >= 1 and asg.max() <= 16)
    out["pipeline_rcm"] = dict(hip.last_rcm_stats)
    print(json.dumps({tag: {k: out[k] for k in ("permute_ms", "pipeline_K16_ms")}}), file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-shaped", type=int, default=1_000_000)
    ap.add_argument("--deg", type=int, default=10)
    ap.add_argument("--n-banded", type=int, default=5_000_000)
    ap.add_argument("--n-python", type=int, default=100_000)
    ap.add_argument("--narrow", default="1048576,256,0", help="values of the option rcm_narrow that permute_plaid is timed with")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--off-reps", type=int, default=1, help="repetitions with rcm_narrow = 0 (one launch chain and readback per level)")
    ap.add_argument("--skip", default="", help="comma list of shaped, symmetrised, banded, python")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_rcm.json"))
    args = ap.parse_args()
    narrows = [int(x) for x in args.narrow.split(",")]
    skip = set(args.skip.split(","))
    dev = torch.device("cuda", 0)
    hip = cp.get_backend()
    default_narrow = DEFAULT_NARROW
    out = {"device": torch.cuda.get_device_name(0), "rcm_narrow_values": narrows}
    try:
        warm = host_matrix(2000, *banded_dev(2000, 4, 0.5, 7, dev))  # code objects of both walks, both regimes and the pipeline
        for nv in (0, 1 << 20):
            hip.set_option("rcm_narrow", nv)
            cp.partition_plaid(warm, 4, PIPELINE, backend=hip)
            cp.permute_plaid(warm, cp.CuthillMcKeePermuter(assumesymmetry=True), backend=hip)
        n = args.n_shaped
        colptr, rowval = gen_suitesparse_shaped(n, args.deg * n, 0xDEADBEEF + 2, dev)
        if "shaped" not in skip:
            out["suitesparse_shaped"] = measure(hip, "suitesparse_shaped", host_matrix(n, colptr, rowval), narrows, args.reps, args.off_reps)
        if "symmetrised" not in skip:
            out["suitesparse_shaped_symmetrised"] = measure(hip, "suitesparse_shaped_symmetrised", host_matrix(n, *symmetrised(colptr, rowval, n)),
                                                            narrows, args.reps, args.off_reps)
        del colptr, rowval
        if "banded" not in skip:
            n = args.n_banded
            out["banded"] = measure(hip, "banded", host_matrix(n, *banded_dev(n, 16, 0.5, 0xDEADBEEF + 4, dev)), narrows, args.reps, args.off_reps)
        if "python" not in skip:
            from rcm_model import rcm_keys, bip_graph
            n = args.n_python
            A = host_matrix(n, *banded_dev(n, 16, 0.5, 0xDEADBEEF + 4, dev))
            g = bip_graph(A, cp.adjointpattern(A, backend=hip))
            t0 = time.perf_counter(); _, trees, levels = rcm_keys(*g); t = time.perf_counter() - t0
            hip.set_option("rcm_narrow", default_narrow)
            td, _ = clock(lambda: cp.permute_plaid(A, RCM, backend=hip))
            out["python_key_formulation"] = {"family": "banded", "n": n, "nnz": A.nnz, "python_ms": round(t * 1e3, 1), "trees": trees, "levels": levels,
                                             "device_ms_same_matrix": round(td * 1e3, 2), "device": dict(hip.last_rcm_stats)}
    finally:
        hip.set_option("rcm_narrow", default_narrow)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
