#!/usr/bin/env python3
"""Generate tests/golden/rcm.json: the permutations permute_plaid(A, CuthillMcKeePermuter(reverse)) of the reference's loops as
tests/rcm_model.py restates them (model A), on the three matrices of test/test_CuthillMcKee.jl (tests/golden/matrices.json).

    python tools/make_golden_rcm.py      (CPU only)
"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from util import golden_matrices
from rcm_model import permute_plaid_model

NAMES = ("HB/can_292", "HB/west0132", "LPnetlib/lp_etamacro")


def main():
    mats = golden_matrices()
    out = {}
    for name in NAMES:
        for reverse in (False, True):
            iprm, jprm, sym, trees = permute_plaid_model(mats[name], reverse=reverse)
            out[f"{name},reverse={int(reverse)}"] = {"rowprm": iprm.tolist(), "colprm": jprm.tolist(), "symmetric": bool(sym), "trees": int(trees)}
    path = os.path.join(ROOT, "tests", "golden", "rcm.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
