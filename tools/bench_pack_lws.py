#!/usr/bin/env python3
"""Timing of pack_stripe(A, DynamicTotalChunker(ConstrainedCost(AffineConnectivityModel(0,0,0,1), VertexCount(), n / 4))) -- the
reference's own benchmark of the method (bin/test_table_constrained_chunks.jl:40) -- on the bench-shaped pattern (nnz = deg * n):
the on-line divide and conquer (csrc/chunk_lws.hip) with its chunk_lws time and launch count, the one-wave kernel at a small n
(cp_set_option("lws", 0)) and the CPU oracle up to the largest n it finishes in about --oracle-s seconds.  One JSON line."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import numpy as np, torch
import cpamd
cp = cpamd.load()
from bench import gen_suitesparse_shaped


def matrix(n, deg, dev):
    colptr, rowval = gen_suitesparse_shaped(n, deg * n, 0xDEADBEEF + 2, dev)
    return cp.SparseMatrixCSC(n, n, colptr.cpu().numpy(), rowval.cpu().numpy())


def method(n):
    return cp.DynamicTotalChunker(cp.ConstrainedCost(cp.AffineConnectivityModel(0, 0, 0, 1), cp.VertexCount(), max(n // 4, 1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="1000000,10000000")
    ap.add_argument("--deg", type=int, default=10)
    ap.add_argument("--one-wave-n", type=int, default=20000)
    ap.add_argument("--oracle-ns", default="5000,10000,20000,40000")
    ap.add_argument("--oracle-s", type=float, default=60.0)
    ap.add_argument("--opt", action="append", default=[])
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    hip = cp.get_backend()
    for kv in args.opt:
        k, v = kv.split("="); assert hip.set_option(k, int(v)) == 0
    out = {"method": "DynamicTotalChunker(ConstrainedCost(AffineConnectivityModel(0,0,0,1), VertexCount(), n/4))", "deg": args.deg, "lws": []}
    for n in [int(x) for x in args.ns.split(",") if x]:
        A = matrix(n, args.deg, dev)
        cp.pack_stripe(A, method(n), backend=hip)            # warm: counters, link arrays, pool
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        P = cp.pack_stripe(A, method(n), backend=hip)
        dt = time.perf_counter() - t0
        hip.prof_reset(); hip.prof_enable(True)
        cp.pack_stripe(A, method(n), backend=hip)
        hip.prof_enable(False)
        pr = hip.prof_get()["chunk_lws"]
        out["lws"].append({"n": n, "nnz": int(A.nnz), "w_max": n // 4, "seconds": round(dt, 4), "chunk_lws_ms_profiled": round(pr["ms"], 2),
                           "chunk_lws_launches": pr["launches"], "chunks": P.K, "total_value": int(cp.total_value(A, P, cp.AffineConnectivityModel(0, 0, 0, 1), backend=hip))})
        print(json.dumps(out["lws"][-1]), file=sys.stderr, flush=True)
        del A
    n = args.one_wave_n
    A = matrix(n, args.deg, dev)
    t0 = time.perf_counter(); P1 = cp.pack_stripe(A, method(n), backend=hip); t_lws = time.perf_counter() - t0
    hip.set_option("lws", 0)
    try:
        t0 = time.perf_counter(); P0 = cp.pack_stripe(A, method(n), backend=hip); t_one = time.perf_counter() - t0
    finally:
        hip.set_option("lws", 1)
    assert P0 == P1
    out["one_wave"] = {"n": n, "nnz": int(A.nnz), "seconds": round(t_one, 4), "lws_seconds": round(t_lws, 4)}
    print(json.dumps(out["one_wave"]), file=sys.stderr, flush=True)
    import orc_binding
    orc = orc_binding.OracleBackend()
    out["oracle"] = []
    for n in [int(x) for x in args.oracle_ns.split(",") if x]:
        A = matrix(n, args.deg, dev)
        t0 = time.perf_counter(); Po = cp.pack_stripe(A, method(n), backend=orc); t = time.perf_counter() - t0
        assert Po == cp.pack_stripe(A, method(n), backend=hip)
        out["oracle"].append({"n": n, "seconds": round(t, 3)})
        print(json.dumps(out["oracle"][-1]), file=sys.stderr, flush=True)
        if t * 4.5 > args.oracle_s:                           # the next n (x2) would take about 4 x as long
            break
    print(json.dumps(out))


if __name__ == "__main__":
    main()
