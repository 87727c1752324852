#!/usr/bin/env python3
"""Timing of the greedy chunkers (csrc/chunk_greedy.hip): pack_stripe(A, StrictChunker(8)) and pack_stripe(A, OverlapChunker(0.9, 8))
-- the methods test/runbenchmarks.jl:34-35 benchmarks -- on the config-3 family (suitesparse_shaped, nnz = deg * n) and on the
config-4 banded family, and pack_plaid(A, AlternatingPacker(OverlapChunker(0.9, 8), OverlapChunker(0.9, 8))) on the banded one.
Per call: ms (host clock around the call, which ends in a stream sync and includes the copy of the split vector to the host), the
kernels' own ms from the profile slots, and the fraction of 8 TB/s on the compulsory bytes (8 (n + 1) + 4 nnz read, 8 (K + 1)
written).  One JSON line."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np, torch
import cpamd
cp = cpamd.load()
from bench import gen_suitesparse_shaped
from bench_configs import banded_dev

HBM = 8e12
SLOTS = ("chunk_col_neq", "chunk_overlap_next", "chunk_orbit", "chunk_compact")


def compulsory(n, nnz, K):
    return 8 * (n + 1) + 4 * nnz + 8 * (K + 1)


def timed(hip, f, reps):
    f()                                                       # warm: code objects, pool, link arrays
    best = 1e30
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter(); K = f(); best = min(best, time.perf_counter() - t0)
    hip.prof_reset(); hip.prof_enable(True)
    f()
    hip.prof_enable(False)
    pr = hip.prof_get()
    return best, K, {k: round(pr[k]["ms"], 3) for k in SLOTS if pr[k]["launches"]}


def stripe_lines(hip, tag, n, nnz, h, reps):
    spl, Kout, nn = np.zeros(n + 1, dtype=np.int64), np.zeros(1, dtype=np.int64), np.zeros(n, dtype=np.int64)

    def strict():
        assert hip.pack_strict(h, 8, spl, Kout) == 0, hip.last_error()
        return int(Kout[0])

    def overlap(nets=None):
        assert hip.pack_overlap(h, 0.9, 8, spl, Kout, nets) == 0, hip.last_error()
        return int(Kout[0])
    out = {}
    for name, f in (("StrictChunker(8)", strict), ("OverlapChunker(0.9, 8)", overlap), ("OverlapChunker(0.9, 8), n_nets", lambda: overlap(nn))):
        hip.set_option("stat_reset", 1)
        t, K, slots = timed(hip, f, reps)
        by = compulsory(n, nnz, K)
        out[name] = {"family": tag, "n": n, "nnz": nnz, "chunks": K, "ms": round(t * 1e3, 3), "kernel_ms": slots, "compulsory_MB": round(by / 1e6, 1),
                     "fraction_of_8TBs": round(by / t / HBM, 5), "fraction_of_8TBs_kernels": round(by / (sum(slots.values()) * 1e-3) / HBM, 5),
                     "width_ok": bool(spl[0] == 1 and spl[K] == n + 1 and np.all(np.diff(spl[:K + 1]) >= 1) and np.all(np.diff(spl[:K + 1]) <= 8))}
        if name.startswith("Overlap"):
            out[name]["intersections_per_call"] = hip.get_stat("overlap_isect") // (reps + 2)
        print(json.dumps({name: out[name]}), file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n3", type=int, default=10_000_000)
    ap.add_argument("--deg", type=int, default=10)
    ap.add_argument("--n4", type=int, default=5_000_000)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    hip = cp.get_backend()
    out = {}
    n = args.n3
    colptr, rowval = gen_suitesparse_shaped(n, args.deg * n, 0xDEADBEEF + 2, dev)
    h = hip.csr_from_device(n, n, rowval.numel(), colptr.data_ptr(), rowval.data_ptr())
    out["cfg3"] = stripe_lines(hip, "suitesparse_shaped", n, int(rowval.numel()), h, args.reps)
    hip.csr_destroy(h)
    del colptr, rowval
    n = args.n4
    colptr, rowval = banded_dev(n, 16, 0.5, 0xDEADBEEF + 4, dev)
    nnz = int(rowval.numel())
    h = hip.csr_from_device(n, n, nnz, colptr.data_ptr(), rowval.data_ptr())
    out["cfg4"] = stripe_lines(hip, "banded", n, nnz, h, args.reps)
    hip.csr_destroy(h)
    # pack_plaid through the public entry: A and its adjoint stay resident between the two sweeps
    A = cp.SparseMatrixCSC(n, n, colptr.cpu().numpy(), rowval.cpu().numpy())
    del colptr, rowval
    t0 = time.perf_counter(); T = cp.adjointpattern(A, backend=hip); t_adj = time.perf_counter() - t0
    meth = cp.AlternatingPacker(cp.OverlapChunker(0.9, 8), cp.OverlapChunker(0.9, 8))
    res = []

    def plaid():
        res[:] = cp.pack_plaid(A, meth, adj_A=T, backend=hip)
        return res[0].K + res[1].K
    t, K2, slots = timed(hip, plaid, args.reps)
    by = compulsory(n, nnz, res[1].K) + compulsory(n, nnz, res[0].K)
    out["cfg4"]["pack_plaid(AlternatingPacker(OverlapChunker(0.9, 8) x 2))"] = {
        "n": n, "nnz": nnz, "chunks_Pi": res[0].K, "chunks_Phi": res[1].K, "ms": round(t * 1e3, 3), "kernel_ms": slots,
        "adjointpattern_with_download_ms": round(t_adj * 1e3, 1), "compulsory_MB": round(by / 1e6, 1), "fraction_of_8TBs": round(by / t / HBM, 5)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
