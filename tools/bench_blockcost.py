#!/usr/bin/env python3
"""Timing of the 2-D block cost on the quotient pattern (csrc/blockcost.hip), on the `banded` generator of tests/synth.py
(half-bandwidth 16, fill 0.5):

    mdl     = BlockComponentCostModel(1, 3, (1, x -> x), (1, x -> x))                 Int64
    Pi      = pack_stripe(adjointpattern(A), EquiChunker(4))
    chunker = DynamicTotalChunker(ConstrainedCost(mdl, VertexCount(), 8))

    pack    : pack_stripe(A, chunker, Pi)
    value   : total_value(A, Phi, mdl, Pi) of its result Phi
    plaid   : pack_plaid(A, AlternatingPacker(EquiChunker(4), chunker, chunker))

Host clock around calls that end in a stream synchronise, best of --reps after a warm call.  Each call is also timed under
cp_set_option("force_brute", 1) -- the stateful one-wave kernels, the only path before blockcost.hip -- once per size, at the sizes
of --cross-ns for as long as ten times the previous size's slowest call stays within --brute-limit seconds (the one-wave kernels are
linear in n; a size left out says so).  One more profiled pack call gives the per-kernel split (quotient build, link build of the
quotient, window table, scan).  Writes the JSON to --out and prints it as one line."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch
import cpamd
cp = cpamd.load()
from util import banded

MODEL = cp.BlockComponentCostModel(1, 3, (1, lambda x: x), (1, lambda x: x))
CHUNKER = cp.DynamicTotalChunker(cp.ConstrainedCost(MODEL, cp.VertexCount(), 8))
PACKER = cp.AlternatingPacker(cp.EquiChunker(4), CHUNKER, CHUNKER)
SPLIT = ("block_quotient", "link_build", "block_table", "chunker")      # the profile slots of one chunker call; chunker: the (min,+) scan


def timed(f, reps):
    best, out = None, None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, out


def calls(hip, A, Pi):
    """name -> the timed call; value scores the packing of the path that is being timed"""
    state = {}

    def pack():
        state["Phi"] = cp.pack_stripe(A, CHUNKER, Pi, backend=hip)
        return state["Phi"]
    return {"pack": pack, "value": lambda: cp.total_value(A, state["Phi"], MODEL, Pi, backend=hip),
            "plaid": lambda: cp.pack_plaid(A, PACKER, backend=hip)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="10000,100000,1000000,5000000")
    ap.add_argument("--cross-ns", default="10000,100000,1000000")
    ap.add_argument("--brute-limit", type=float, default=60.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_blockcost.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "no GPU: nothing is measured without one"
    hip = cp.get_backend()
    cross = [int(x) for x in args.cross_ns.split(",") if x]
    out = {"model": "BlockComponentCostModel(1, 3, (1, x -> x), (1, x -> x)), Int64", "Pi": "pack_stripe(adjointpattern(A), EquiChunker(4))",
           "method": "DynamicTotalChunker(ConstrainedCost(model, VertexCount(), 8))", "plaid": "AlternatingPacker(EquiChunker(4), method, method)",
           "matrix": "banded(n, 16, 0.5, seed = n)", "reps": args.reps, "brute_limit_seconds": args.brute_limit, "sizes": []}
    brute_prev = 0.0                    # the slowest force_brute call of the last size that ran them
    for n in [int(x) for x in args.ns.split(",") if x]:
        A = banded(n, 16, 0.5, n)
        Pi = cp.pack_stripe(cp.adjointpattern(A, backend=hip), cp.EquiChunker(4))
        row = {"n": n, "nnz": int(A.nnz), "row_parts": Pi.K}
        fs = calls(hip, A, Pi)
        results = {}
        for name, f in fs.items():
            f()                                                             # warm: code objects, the pool
            row[name + "_seconds"], results[name] = timed(f, args.reps)
        row["chunks"] = results["pack"].K
        hip.set_option("stat_reset", 0)
        hip.prof_reset(); hip.prof_enable(True)
        fs["pack"]()
        hip.prof_enable(False)
        prof = hip.prof_get()
        row["pack_profiled_ms"] = {k: round(prof[k]["ms"], 3) for k in SPLIT}
        row["pack_profiled_launches"] = {k: prof[k]["launches"] for k in SPLIT}
        assert hip.get_stat("blockcost_scan_packs") == 1
        if n in cross and 10.0 * brute_prev <= args.brute_limit:
            hip.set_option("force_brute", 1)
            try:
                for name, f in fs.items():
                    row[name + "_force_brute_seconds"], lit = timed(f, 1)
                    assert lit == results[name], (n, name, "the two paths disagree")
            finally:
                hip.set_option("force_brute", 0)
            brute_prev = max(row[k + "_force_brute_seconds"] for k in fs)
        elif n in cross:
            row["force_brute"] = f"not run: ten times the {brute_prev:.1f} s of the previous size exceeds {args.brute_limit:.0f} s"
        out["sizes"].append({k: (round(v, 5) if isinstance(v, float) else v) for k, v in row.items()})
        print(json.dumps(out["sizes"][-1]), file=sys.stderr, flush=True)
        with open(args.out, "w") as fh:                                     # (after every size: a run that is cut short keeps its rows)
            json.dump(out, fh, indent=1)
            fh.write("\n")
        del A, fs, results
    print(json.dumps(out))


if __name__ == "__main__":
    main()
