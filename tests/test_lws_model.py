"""The executable specification of csrc/chunk_lws.hip (tests/lws_model.py): the staircase decomposition covers every feasible cell
exactly once, and the on-line divide and conquer with lexicographic minima equals the literal recurrence of DynamicChunker.jl:20-56
(costs AND smallest-j split points) on connectivity, hyperedge-cut and work costs over golden and seeded patterns."""
import numpy as np
import pytest

from util import cp, sprand, golden_matrices, suitesparse_shaped, banded
import lws_model as lm

COSTS = [("conn", (0, 0, 0, 1)), ("conn", (0, 3, 1, 3)), ("conn", (-7, 0, 0, 1)), ("work", (0, 0, 0)), ("work", (-3, 1, 0)),
         ("hedge", (0, 1, 1, 1, 3))]


def patterns():
    rng = np.random.default_rng(77)
    out = [sprand(m, n, p, rng) for (m, n, p) in [(1, 1, 0.5), (3, 5, 0.5), (8, 16, 0.3), (12, 31, 0.15), (20, 40, 0.1), (30, 70, 0.06)]]
    out += [suitesparse_shaped(90, 4, 7), banded(80, 3, 0.5, 3), golden_matrices()["LPnetlib/lpi_itest6"]]
    return out


def weights(A):
    n = A.n
    out = [("none", [0] * (n + 1))]
    for w in sorted({1, 2, 17, 63, 64, 65, max(n // 4, 1), max(n, 1)}):
        out.append((f"width {w}", lm.lo_width(n, w)))
    deg = int(np.diff(A.colptr).max(initial=0))
    budget = max(deg, A.nnz // 6, 1)
    out.append(("pins (0,0,1)", lm.lo_budget(A, 0, 0, 1, budget)))
    out.append(("pins (0,1,1)", lm.lo_budget(A, 0, 1, 1, budget + max(n // 5, 1))))
    return out


def test_decomposition_covers_each_feasible_cell_once():
    rng = np.random.default_rng(3)
    for trial in range(60):
        n = int(rng.integers(1, 60))
        steps = np.sort(rng.integers(0, n + 1, size=n + 1))
        lo = [min(int(v), r) for r, v in enumerate(steps)]
        lo = list(np.maximum.accumulate(lo))
        ja = int(rng.integers(0, n))
        jb = int(rng.integers(ja, n))
        ra, rb = jb + 1, n
        for stair in (0, 4):
            rects = []
            lm.push_rects(ja, jb, ra, rb, lo, rects, stair)
            seen = {}
            for (a, b, x, y, st) in rects:
                for r in range(x, y + 1):
                    assert st or lo[r] <= a, "a rectangle must be fully feasible"
                    for p in range(max(a, lo[r]) if st else a, b + 1):
                        seen[(r, p)] = seen.get((r, p), 0) + 1
            want = {(r, p) for r in range(ra, rb + 1) for p in range(max(ja, lo[r]), jb + 1)}
            assert set(seen) == want
            assert all(v == 1 for v in seen.values())


@pytest.mark.parametrize("L,stair", [(1, 0), (4, 0), (16, 0), (4, 8)])
def test_divide_and_conquer_equals_the_literal_recurrence(L, stair):
    for A in patterns():
        n = A.n
        for kind, params in COSTS:
            f = lm.cost_fn(A, kind, params)
            for name, lo in weights(A):
                if any(lo[r] >= r for r in range(1, n + 1)):
                    continue                              # infeasible budget: the @assert of both paths
                want = lm.brute(n, f, lo)
                rects = []
                got = lm.solve(n, f, lo, L=L, rects=rects, stair=stair)
                assert got == want, (A, kind, params, name, L, stair)


def test_leftmost_argmin_non_increasing_in_full_rectangles():
    """the property the rectangle divide and conquer rests on, checked cell by cell on real costs"""
    for A in patterns()[:7]:
        n = A.n
        for kind, params in COSTS:
            f = lm.cost_fn(A, kind, params)
            cst, _ = lm.brute(n, f, [0] * (n + 1))
            for jb in range(0, n - 1, 3):
                ja = jb // 2
                prev = None
                for r in range(jb + 1, n + 1):
                    vals = [(cst[p] + f(p, r), p) for p in range(ja, jb + 1)]
                    arg = min(vals)[1]
                    assert prev is None or arg <= prev, (A, kind, params, ja, jb, r)
                    prev = arg
