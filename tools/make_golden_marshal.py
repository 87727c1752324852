#!/usr/bin/env python3
"""Generate tests/golden/marshal.json: what the host layer hands to the C ABI for a spread of cost models -- the bytes of
the cp_model_t (pointer fields zeroed) and every table it points into -- so that a change to models.py / api.py that is
meant to leave the marshalling alone can be held to it byte for byte (tests/test_abi_and_host.py).

    python tools/make_golden_marshal.py      (CPU only, no library call)
"""
import ctypes as C
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np
import cpamd
cp = cpamd.load()
M = cp.models
PATH = os.path.join(ROOT, "tests", "golden", "marshal.json")


def dump(mm):
    """a Marshalled as JSON: the struct's bytes with its pointers zeroed, and the kept tables in order"""
    if mm is None:
        return None
    s = M.cp_model_t.from_buffer_copy(bytes(mm.struct))
    s.alpha_k = None
    for c in (s.alpha_row, s.alpha_col, *s.beta_row, *s.beta_col):
        c.table = None
    words = np.frombuffer(bytes(s), dtype="<u8")             # the struct as 8-byte words; only the non-zero ones are stored
    return {"size": C.sizeof(s), "words": [[int(i), f"{int(words[i]):x}"] for i in np.flatnonzero(words)],
            "tables": [[a.dtype.name, a.tolist()] for a in mm.keep]}


def via_api(f, stack_method=False, m=7, n=9):
    """api._marshal on an m x n pattern (only the shape matters to marshalling; m != n tells the row tables from the column ones)"""
    A = cp.SparseMatrixCSC(m, n, np.ones(n + 1, dtype=np.int64), np.zeros(0, dtype=np.int64))
    _, mm, wm, wi, wf, rp, _ = cp.api._marshal(A, f, None, stack_method)
    assert rp is None
    return {"model": dump(mm), "weight": dump(wm), "wi": wi, "wf": wf}


def cases():
    """(name, thunk -> JSON value)"""
    vc = M.VertexCount
    sq = lambda w: w * w + 1
    out = []
    affine = [("work", M.AffineWorkModel, 3), ("connectivity", M.AffineConnectivityModel, 4), ("hyperedge", M.AffineHyperedgeCutModel, 5),
              ("primary", M.AffinePrimaryConnectivityModel, 5), ("secondary", M.AffineSecondaryConnectivityModel, 5),
              ("sym_connectivity", M.AffineSymmetricConnectivityModel, 5), ("mono_sym", M.AffineMonotonizedSymmetricConnectivityModel, 5),
              ("sym_edge_cut", M.AffineSymmetricEdgeCutModel, 4)]
    for name, cls, k in affine:
        ints = [2, 10, 1, 100, 7][:k]
        out.append((f"{name}/i64", lambda cls=cls, a=ints: via_api(cls(*a))))
        out.append((f"{name}/f64", lambda cls=cls, a=ints: via_api(cls(*[a[0] + 0.5] + a[1:]))))
    out += [
        ("power_work/ints_forced_f64", lambda: via_api(M.PowerWorkModel(1, 2, 3, 2))),
        ("convex_work", lambda: via_api(M.ConvexWorkModel(0.5, 1, 0.25), True)),
        ("work/alpha_k_i64", lambda: via_api(M.AffineWorkModel(0, 10, 1, alpha_k=[3, 1, 4]))),
        ("connectivity/alpha_k_f64", lambda: via_api(M.AffineConnectivityModel(0, 10, 1, 100, alpha_k=[0.5, 2, 7]))),
        ("connectivity/alpha_k_promotes_ints", lambda: via_api(M.AffineConnectivityModel(0.0, 10, 1, 100, alpha_k=(1, 2)))),
        ("hyperedge/alpha_k", lambda: via_api(M.AffineHyperedgeCutModel(0, 1, 2, 3, 4, alpha_k=np.array([5, 6])))),
        ("primary/alpha_k", lambda: via_api(M.AffinePrimaryConnectivityModel(0, 1, 2, 3, 4, alpha_k=[9]))),
        ("mono_sym/alpha_k", lambda: via_api(M.AffineMonotonizedSymmetricConnectivityModel(1, 2, 3, 4, 2, alpha_k=[1, 2, 3]))),
        ("mono_sym/converted_i64", lambda: via_api(M.AffineMonotonizedSymmetricConnectivityModel(M.AffineSymmetricConnectivityModel(1, 2, 3, 0, 9)))),
        ("mono_sym/converted_f64", lambda: via_api(M.AffineMonotonizedSymmetricConnectivityModel(M.AffineSymmetricConnectivityModel(1.5, 9, 2, 0, 4)))),
        # the column block model: callables, tuples and constants; the four tabulation ranges of api._w_table_for
        ("colblock/callable", lambda: via_api(M.ColumnBlockComponentCostModel(3, lambda w: 1 + w))),
        ("colblock/callable/stack", lambda: via_api(M.ColumnBlockComponentCostModel(3, lambda w: 1 + w), True)),
        ("colblock/callable/vertexcount4", lambda: via_api(M.ConstrainedCost(M.ColumnBlockComponentCostModel(sq, lambda w: 1 + w), vc(), 4))),
        ("colblock/callable/vertexcount4/stack", lambda: via_api(M.ConstrainedCost(M.ColumnBlockComponentCostModel(sq, lambda w: 1 + w), vc(), 4), True)),
        ("colblock/callable/work_weight", lambda: via_api(M.ConstrainedCost(M.ColumnBlockComponentCostModel(sq, 2), M.AffineWorkModel(0, 1, 0), 4))),
        ("colblock/callable/work_weight_f64/stack", lambda: via_api(M.ConstrainedCost(M.ColumnBlockComponentCostModel(sq, 2), M.AffineWorkModel(0.0, 1, 0), 3.5), True)),
        ("colblock/feasible_weight", lambda: via_api(M.ConstrainedCost(M.ColumnBlockComponentCostModel(sq, 2), M.FeasibleCost(), 4))),
        ("colblock/tuple_const_f64", lambda: via_api(M.ColumnBlockComponentCostModel((1, 2.5, 4), 2, dtype=float))),
        ("colblock/preset_w_table", lambda: via_api(M.ColumnBlockComponentCostModel(sq, sq, w_table=3))),
        ("connectivity/vertexcount4", lambda: via_api(M.ConstrainedCost(M.AffineConnectivityModel(0, 10, 1, 100), vc(), 4))),
        # the block model: row tables run to m + 1 unless u_table is preset (then the model's own w_table / u_table are not replaced)
        ("block/callables", lambda: via_api(M.BlockComponentCostModel(sq, lambda w: 2 * w, (sq, 3), (lambda w: w + 5, (1, 2, 3))))),
        ("block/callables/stack", lambda: via_api(M.BlockComponentCostModel(sq, lambda w: 2 * w, (sq, 3), (lambda w: w + 5, (1, 2, 3))), True)),
        ("block/callables/vertexcount3/stack", lambda: via_api(M.ConstrainedCost(M.BlockComponentCostModel(sq, sq, (sq,), (sq,)), vc(), 3), True)),
        ("block/preset_u_table", lambda: via_api(M.BlockComponentCostModel(sq, sq, (sq,), (sq,), u_table=4))),
        ("block/preset_u_table/stack", lambda: via_api(M.BlockComponentCostModel(sq, sq, (sq,), (sq,), u_table=4), True)),
        ("block/preset_w_table_only", lambda: via_api(M.BlockComponentCostModel(sq, sq, (sq,), (sq,), w_table=2))),
        ("block/consts_tuples_f64", lambda: via_api(M.BlockComponentCostModel(1.5, (1, 2), (2, (3, 4.5)), (1, 1), dtype=float))),
        # Model.marshal called directly, as tools and bound_stripe do
        ("direct/colblock(w_table=5,w_lo=-3)", lambda: dump(M.ColumnBlockComponentCostModel(sq, lambda w: 1 + w).marshal(w_table=5, w_lo=-3))),
        ("direct/colblock(own w_table)", lambda: dump(M.ColumnBlockComponentCostModel(sq, 1, w_table=6).marshal())),
        ("direct/block(w_table=5,w_lo=-2)", lambda: dump(M.BlockComponentCostModel(sq, sq, (sq,), (sq,), u_table=3).marshal(w_table=5, w_lo=-2))),
        ("direct/block(own tables)", lambda: dump(M.BlockComponentCostModel(sq, sq, (sq,), (sq,), w_table=4, u_table=2).marshal())),
        ("direct/connectivity(w_table=10)", lambda: dump(M.AffineConnectivityModel(0, 10, 1, 100).marshal(w_table=10))),
        ("direct/vertexcount", lambda: dump(vc().marshal())),
        ("direct/feasible", lambda: dump(M.FeasibleCost().marshal())),
    ]
    return out


def main():
    out = {name: fn() for name, fn in cases()}
    with open(PATH, "w") as fh:             # one case per line
        fh.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in out.items()) + "\n}\n")
    print(len(out), "marshalled models,", os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
