"""Self-checks of tests/bellman_audit.py: the sampled rows hold the rows where the rectangle engine changes its path, and the audit has
the power it is used for -- it passes on tables of the literal DP and fails after each of four single-cell mutations.  No GPU."""
import numpy as np
import pytest

import bellman_audit as ba
import plaid_total_model as ptm
import sym_model as sm
from util import cp


@pytest.mark.parametrize("n", [17_001, 250_000])
def test_structural_rows_are_sampled(n):
    rows = set(ba.audit_rows(n, 1024, 7, 32).tolist())
    assert {0, 1, 2, n - 1, n} <= rows
    for c in (256, 1024, 4096, 8192):
        assert {c - 1, c, c + 1} <= rows
    # the column tree by hand: [0, n] and its two children, then every block of the depths 2 and 3 by the rule of lws_decomp.hpp
    jm = n // 2
    assert {jm, jm + 1, jm + 2, jm // 2, jm // 2 + 1, jm // 2 + 2, (jm + 1 + n) // 2, (jm + 1 + n) // 2 + 1, (jm + 1 + n) // 2 + 2} <= rows
    blocks, mids = [(0, n)], []
    for depth in range(4):
        mids += [(ja + jb) // 2 for ja, jb in blocks]
        blocks = [b for ja, jb in blocks for b in ((ja, (ja + jb) // 2), ((ja + jb) // 2 + 1, jb))]
    assert len(mids) == 15 and all(b - a >= 1024 for a, b in blocks)              # (all fifteen are split at these sizes)
    assert all({m, m + 1, m + 2} <= rows for m in mids)
    assert len(rows) >= 5 + 12 + 45 - 6 and max(rows) == n and min(rows) == 0
    assert ba.audit_rows(n, 1024, 7, 32).tolist() == sorted(rows)
    assert set(ba.audit_rows(n, 1024, 8, 32).tolist()) != rows                      # the seed moves the random rows only
    assert set(ba.structural_rows(n, 1024).tolist()) <= set(ba.audit_rows(n, 1024, 8, 0).tolist())


def test_a_narrow_tree_stops_splitting():
    assert ba.tree_rows(100, 1024) == [] and ba.tree_rows(2000, 1024) == [1000, 1001, 1002]
    assert ba.audit_rows(3, 1024, 1, 0).tolist() == [0, 1, 2, 3]


def _sym_case():
    from test_gpu_symmetric import pattern, tables
    n, K, mdl = 257, 5, cp.AffineSymmetricEdgeCutModel(0, 0, 0, 1)
    A, T = pattern(n, "holes"), tables(n, "holes")
    cst, ptr = [sm.cost_table(T, mdl, 1)[0, :].copy()], [np.zeros(n + 1, dtype=np.int64)]
    for k in range(2, K + 1):
        c, p = sm.brute.layer(cst[-1], sm.cost_table(T, mdl, k))
        cst.append(c); ptr.append(p)
    S = sm.Sym(A, mdl)
    return n, K, np.stack(cst, axis=1), np.stack(ptr, axis=1) + 1, S.row, ba.same_for_all_k(S.column), S.column


def _primary_case():
    import test_gpu_plaid_total as g
    n, K, mdl = 257, 5, g.MODELS["i"][5]
    T = g.counts(n, "map")
    cst, ptr = ptm.literal_dp(lambda k: T.table(mdl, k), K, n)
    C = ptm.PrimaryCols(T.A, T.Pi, mdl)
    return n, K, np.stack(cst, axis=1), np.stack(ptr, axis=1) + 1, C.row, C.column, C.column


@pytest.mark.parametrize("case", [_sym_case, _primary_case], ids=["symmetric", "primary"])
def test_audit_passes_on_the_literal_dp_and_fails_on_four_mutations(case):
    n, K, cst, ptr, row_of, column_of, fresh_column = case()
    rows = ba.audit_rows(n, 64, 3, 16)
    counts = ba.audit(ptr, cst, K, row_of, column_of, rows)
    assert counts["cells"] == len(rows) * (K - 2) + 1 and counts["tied"] >= 1, counts
    if case is _primary_case:
        assert counts["interior"] >= 1, counts

    # a cell with two or more minimisers and one with a non-minimiser, both at audited rows of a full layer
    tied = plain = None
    for r in rows[::-1]:
        for k in range(2, K):
            v = cst[:r + 1, k - 2] + fresh_column(int(r) + 1, k)
            at = np.nonzero(v == v.min())[0]
            if at.size >= 2 and tied is None:
                tied = (int(r), k, int(at[-2]))
            if at.size <= r and plain is None:
                plain = (int(r), k, int(np.nonzero(v != v.min())[0][-1]))
    assert tied is not None and plain is not None

    def fails(what, r, k, value, match):
        table = {"cst": cst, "ptr": ptr}[what]
        keep = table[r, k - 1]
        table[r, k - 1] = value
        try:
            with pytest.raises(AssertionError, match=match):
                ba.audit(ptr, cst, K, row_of, column_of, rows)
        finally:
            table[r, k - 1] = keep

    r, k, _ = plain
    fails("cst", r, k, cst[r, k - 1] + 1, "cst")                                 # a cost off by one unit, either way
    fails("cst", r, k, cst[r, k - 1] - 1, "cst")
    fails("cst", n, K, cst[n, K - 1] + 1, "cst")                                 # ... and in the last layer's one row
    r, k, second = tied
    fails("ptr", r, k, second + 1, "ptr")                                        # the smaller of two equal minimisers
    r, k, other = plain
    fails("ptr", r, k, other + 1, "ptr")                                         # a non-minimiser, the cost left as it is
    off = int(rows[len(rows) // 2]) + 1                                          # layer 1 is checked in every cell: off the sampled rows too
    assert off not in set(rows.tolist())
    fails("cst", off, 1, cst[off, 0] + 1, "layer 1 cst")
    fails("ptr", off, 1, 2, "layer 1 ptr")
    assert ba.audit(ptr, cst, K, row_of, column_of, rows) == counts             # every mutation was undone
