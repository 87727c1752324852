"""Executable statement (plain Python, small n) of what csrc/sym_total.hip adds to tests/budget_model.py: the unconstrained layer as
the two-staircase layer with a(r) = 0, b(r) = r, and the grouping of its rectangles by the depth of the column tree.

0-based indices as in budget_model: row r = j' - 1, candidate p = j - 1."""
import math

import budget_model as bm


def layer(W, F, scan_cells=0, scan_cols=0, stair=1, blocks=None):
    """one unconstrained layer over all rows: {r: (cost, p)}, ties to the largest p"""
    n = F.shape[0] - 1
    return bm.layer(W, F, 0, n, 0, n, [0] * (n + 1), scan_cells=scan_cells, scan_cols=scan_cols, stair=stair, blocks=blocks)


def triangle_blocks(n, stair, rlo=0):
    """the decomposition of the rows rlo .. n of the triangle 0 <= p <= r <= n"""
    a = {r: 0 for r in range(rlo, n + 1)}
    b = {r: r for r in range(rlo, n + 1)}
    out = []
    bm.push_blocks(0, n, rlo, n, a, b, out, stair)
    return out, a, b


def depth_of(n, ja, jb):
    """how many halvings lead from the candidates [0, n] to the block [ja, jb] of the column tree (push_blocks splits at (ja + jb) // 2)"""
    lo, hi, d = 0, n, 0
    while (lo, hi) != (ja, jb):
        assert lo < hi and lo <= ja and jb <= hi, "not a block of the tree"
        jm = (lo + hi) // 2
        lo, hi = (lo, jm) if jb <= jm else (jm + 1, hi)
        d += 1
    return d


def by_depth(n, blocks):
    """{depth: (rectangles, stair scans)} of a decomposition of the triangle"""
    out = {}
    for blk in blocks:
        d = depth_of(n, blk[1], blk[2])
        out.setdefault(d, ([], []))[0 if blk[0] == "rect" else 1].append(blk)
    return out


def launch_cap(n, stair):
    """D (4 L + 2) + 1: D depths of the column tree over the candidates 0 .. n with leaves below `stair` columns, L = ceil(log2(n + 1))
    levels, each at most count + scan + level + fin, one scan launch for the small rectangles and one for the partial rows per depth,
    and the init launch"""
    D, cols = 1, n + 1
    while cols - 1 >= stair:                     # (a block of jb - ja >= stair splits; its larger half has ceil(cols / 2) columns)
        cols = (cols + 1) // 2
        D += 1
    L = math.ceil(math.log2(n + 1))
    return D * (4 * L + 2) + 1
