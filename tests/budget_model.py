"""Executable specification (numpy / plain Python, small n) of csrc/dp_total_budget.hip: one layer of the K-part total-cost DP under
a monotone work budget, decomposed between two staircases, and the K-layer run of csrc/dp_driver.hip around it.

0-based indices: row r = j' - 1, candidate p = j - 1, F[p, r] = cost of the columns [p, r).  Row r of a layer takes its candidates
from [a[r], b[r]], a[r] = max(j0[r], p_lo0), b[r] = min(r, p_hi0), both non-decreasing; the minimum is the smallest value and, among
equals, the LARGEST p (DynamicSplitter.jl:233-246).
"""
import numpy as np


def push_blocks(ja, jb, ra, rb, a, b, out, stair=1):
    """The feasible cells {(r, p) : ja <= p <= jb, ra <= r <= rb, a[r] <= p <= b[r]} as full rectangles ("rect", ja, jb, f1, f2)
    and whole scans of partial rows ("stair", ja, jb, rows), appended to out -- BudgetRun::push."""
    if ja > jb or ra > rb:
        return
    rows = range(ra, rb + 1)
    s = next((r for r in rows if b[r] >= ja), rb + 1)               # the rows that meet the block: a suffix by b ...
    e = next((r for r in reversed(rows) if a[r] <= jb), ra - 1)     # ... and a prefix by a
    if s > e:
        return
    f1 = next((r for r in range(s, e + 1) if b[r] >= jb), e + 1)    # ... those that see all of it
    f2 = next((r for r in range(e, s - 1, -1) if a[r] <= ja), s - 1)
    top, bot = (s, e), (e + 1, e)
    if f1 <= f2:
        out.append(("rect", ja, jb, f1, f2))
        top, bot = (s, f1 - 1), (f2 + 1, e)
    if top[1] < top[0] and bot[1] < bot[0]:
        return
    if jb - ja < stair:
        out.append(("stair", ja, jb, list(range(top[0], top[1] + 1)) + list(range(bot[0], bot[1] + 1))))
        return
    jm = (ja + jb) // 2
    for (x, y) in (top, bot):
        push_blocks(ja, jm, x, y, a, b, out, stair)
        push_blocks(jm + 1, jb, x, y, a, b, out, stair)


def better(cand, best):
    """(cost, p) pairs: smaller cost, or the same cost from a larger p"""
    return best is None or cand[0] < best[0] or (cand[0] == best[0] and cand[1] > best[1])


def scan(val, r, c0, c1):
    best = None
    for p in range(c0, c1 + 1):
        cand = (val(p, r), p)
        if better(cand, best):
            best = cand
    return best


def rect_minima(ja, jb, ra, rb, val, scan_cells=0, scan_cols=0):
    """Row minima of a full rectangle: scanned whole inside the two limits, else by the monotone divide and conquer level by level as
    k_lws_level runs it -- row i = h - 1 + 2 h u searches [opt(i + h), opt(i - h)], the rightmost argmin being non-increasing in r.
    -> {r: (cost, p)}"""
    m, cols = rb - ra + 1, jb - ja + 1
    if cols <= scan_cols and m * cols <= scan_cells:
        return {r: scan(val, r, ja, jb) for r in range(ra, rb + 1)}
    opt, res = {}, {}
    h = 1
    while 2 * h <= m:
        h *= 2
    while h >= 1:
        for i in range(h - 1, m, 2 * h):
            lo = opt[i + h] if i + h < m else ja
            hi = opt[i - h] if i >= h else jb
            best = scan(val, ra + i, lo, max(lo, hi))
            opt[i] = best[1]
            res[ra + i] = best
        h //= 2
    return res


def layer(W, F, rlo, rhi, p_lo0, p_hi0, j0, scan_cells=0, scan_cols=0, stair=1, blocks=None):
    """dp_total_budget_layer: {r: (cost, p)} for the rows rlo .. rhi; blocks (a list) collects the decomposition."""
    a = {r: max(int(j0[r]), p_lo0) for r in range(rlo, rhi + 1)}
    b = {r: min(r, p_hi0) for r in range(rlo, rhi + 1)}
    out = []
    push_blocks(p_lo0, p_hi0, rlo, rhi, a, b, out, stair)
    if blocks is not None:
        blocks.extend(out)
    val = lambda p, r: W[p] + F[p, r]
    best = {r: None for r in range(rlo, rhi + 1)}
    for blk in out:
        if blk[0] == "rect":
            found = rect_minima(blk[1], blk[2], blk[3], blk[4], val, scan_cells, scan_cols)
        else:
            found = {r: scan(val, r, max(a[r], blk[1]), min(b[r], blk[2])) for r in blk[3]}
        for r, cand in found.items():
            if better(cand, best[r]):
                best[r] = cand
    return best


def windows(n, K, j0):
    """column_constraints (DynamicSplitter.jl:144-172) for a monotone weight from its j0 array -- weight_windows of dp_driver.hip;
    1-based j', lists indexed by k = 1 .. K"""
    lo, hi = [0] * (K + 1), [0] * (K + 1)
    jp = n + 1
    for k in range(K, 0, -1):
        lo[k] = jp
        jp = min(jp, int(j0[jp - 1]) + 1)
    j = 1
    for k in range(1, K + 1):
        fit = sum(1 for v in j0 if v <= j - 1)
        hi[k] = max(j, fit)
        j = hi[k]
    return lo, hi


def run(n, K, F_of_k, j0, typemax, **kw):
    """The K-layer run: (feasible, lo[K], hi[K], ptr[n + 1, K], cst[n + 1, K]) in the oracle's layout -- ptr 1-based, 0 and typemax
    outside the windows"""
    lo, hi = windows(n, K, j0)
    F1 = F_of_k(1)
    ptr = np.zeros((n + 1, K), dtype=np.int64)
    cst = np.full((n + 1, K), typemax, dtype=F1.dtype)
    if hi[K] < n + 1:
        return False, lo[1:], hi[1:], ptr, cst
    for r in range(lo[1] - 1, hi[1]):
        cst[r, 0] = F1[0, r]
        ptr[r, 0] = 1
    for k in range(2, K + 1):
        got = layer(cst[:, k - 2], F_of_k(k), lo[k] - 1, hi[k] - 1, lo[k - 1] - 1, hi[k - 1] - 1, j0, **kw)
        for r, (c, p) in got.items():
            cst[r, k - 1] = c
            ptr[r, k - 1] = p + 1
    return True, lo[1:], hi[1:], ptr, cst
