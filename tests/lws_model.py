"""Executable specification (numpy / plain Python, small n) of csrc/chunk_lws.hip: pack_stripe(A, DynamicTotalChunker(...)) as an
on-line divide and conquer over the columns.  Used by the CPU tests to prove that the staircase decomposition covers every feasible
cell once and that the scheme, with lexicographic (cost, p) minima, reproduces the literal recurrence of DynamicChunker.jl:20-56.

0-based indices: row r = j' - 1, candidate p = j - 1, f(p, r) = cost of columns [p, r), lo[r] = j0(j') - 1 (non-decreasing).
"""
import numpy as np


def brute(n, f, lo):
    """DynamicChunker.jl:20-56 as written: j scanned upwards with a strict <  ->  (cst[0..n], spl[0..n]) with spl[r] = j (1-based)."""
    cst = [0] * (n + 1)
    spl = [0] * (n + 1)
    for r in range(1, n + 1):
        best, bj = None, None
        for p in range(lo[r], r):
            c = cst[p] + f(p, r)
            if best is None or c < best:
                best, bj = c, p + 1
        cst[r], spl[r] = best, bj
    return cst, spl


def push_rects(ja, jb, ra, rb, lo, out, stair=0):
    """The feasible cells {(r, p) : ja <= p <= jb, ra <= r <= rb, p >= lo[r]} as full rectangles (ja, jb, ra, rb', False), appended
    to out; a staircase narrower than `stair` columns stays whole: (ja, jb, ra', rb', True) covers [max(lo[r], ja), jb] per row."""
    if ja > jb or ra > rb:
        return
    r1 = ra - 1
    while r1 + 1 <= rb and lo[r1 + 1] <= ja:
        r1 += 1
    r2 = r1
    while r2 + 1 <= rb and lo[r2 + 1] <= jb:
        r2 += 1
    if r1 >= ra:
        out.append((ja, jb, ra, r1, False))
    if r2 > r1 and jb - ja < stair:
        out.append((ja, jb, r1 + 1, r2, True))
    elif r2 > r1 and ja < jb:
        jm = (ja + jb) // 2
        push_rects(jm + 1, jb, r1 + 1, r2, lo, out, stair)
        push_rects(ja, jm, r1 + 1, r2, lo, out, stair)


def lex_less(a, b):
    return b is None or a < b


def rect_minima(ja, jb, ra, rb, val):
    """Row minima of a full rectangle by the monotone divide and conquer, level by level as k_lws_level runs it: row i = h - 1 + 2 h u
    searches [opt(i + h), opt(i - h)] (the leftmost argmin is non-increasing in r).  -> {r: (cost, p)}"""
    m = rb - ra + 1
    opt, res = {}, {}
    h = 1
    while 2 * h <= m:
        h *= 2
    while h >= 1:
        for i in range(h - 1, m, 2 * h):
            a = opt[i + h] if i + h < m else ja
            b = opt[i - h] if i >= h else jb
            best = None
            for p in range(a, b + 1):
                cand = (val(p, ra + i), p)
                if lex_less(cand, best):
                    best = cand
            opt[i] = best[1]
            res[ra + i] = best
        h //= 2
    return res


def solve(n, f, lo, L=4, rects=None, stair=0):
    """The device algorithm: (cst[0..n], spl[0..n]); rects (a list) collects every pushed rectangle."""
    cst = [0] * (n + 1)
    spl = [0] * (n + 1)
    best = [None] * (n + 1)

    def leaf(x, y):
        for r in range(x, y + 1):
            b = best[r]
            for p in range(max(x, lo[r]), r):
                cand = (cst[p] + f(p, r), p)
                if lex_less(cand, b):
                    b = cand
            if r > 0:
                cst[r], spl[r] = b[0], b[1] + 1

    def rec(x, y):
        if y - x + 1 <= L:
            leaf(x, y)
            return
        nb = -(-(y - x + 1) // L)
        mid = x + L * ((nb + 1) // 2) - 1
        rec(x, mid)
        out = []
        push_rects(x, mid, mid + 1, y, lo, out, stair)
        for (ja, jb, ra, rb, st) in out:
            if rects is not None:
                rects.append((ja, jb, ra, rb, st))
            if st:
                found = {r: min((cst[p] + f(p, r), p) for p in range(max(lo[r], ja), jb + 1)) for r in range(ra, rb + 1)}
            else:
                found = rect_minima(ja, jb, ra, rb, lambda p, r: cst[p] + f(p, r))
            for r, cand in found.items():
                if lex_less(cand, best[r]):
                    best[r] = cand
        rec(mid + 1, y)

    rec(0, n)
    return cst, spl


# ---------------------------------------------------------------- costs and weights from the pattern
def counts(A):
    """(pos, nets(p, r), self_nets(p, r)) as functions over the pattern (distinct rows in columns [p, r); rows inside them)"""
    pos = np.asarray(A.colptr, dtype=np.int64) - 1
    rows = [set((np.asarray(A.rowval[pos[c]:pos[c + 1]]) - 1).tolist()) for c in range(A.n)]
    first, last = {}, {}
    for c in range(A.n):
        for i in rows[c]:
            first.setdefault(i, c)
            last[i] = c
    cache = {}

    def nets(p, r):
        if (p, r) not in cache:
            s = set()
            for c in range(p, r):
                s |= rows[c]
            cache[(p, r)] = (len(s), sum(1 for i in s if first[i] >= p and last[i] < r))
        return cache[(p, r)]
    return pos, nets


def cost_fn(A, kind, params):
    """f(p, r) of AffineWorkModel / AffineConnectivityModel / AffineHyperedgeCutModel (WorkCosts.jl:17, ConnectivityCosts.jl:20,
    HyperedgeCutCosts.jl:21) in exact integers"""
    pos, nets = counts(A)

    def f(p, r):
        nv, npins = r - p, int(pos[r] - pos[p])
        base = params[0] + nv * params[1] + npins * params[2]
        if kind == "work":
            return base
        nn, nl = nets(p, r)
        if kind == "conn":
            return base + nn * params[3]
        return base + nl * params[3] + (nn - nl) * params[4]
    return f


def lo_width(n, w):
    return [max(0, r - w) for r in range(n + 1)]


def lo_budget(A, alpha, bv, bp, wmax):
    """first p whose part [p, r) fits alpha + bv nv + bp np <= wmax (k_weight_j0); r + 1 when none does"""
    pos = np.asarray(A.colptr, dtype=np.int64) - 1
    out = []
    for r in range(A.n + 1):
        p = 0
        while p <= r and alpha + (r - p) * bv + int(pos[r] - pos[p]) * bp > wmax:
            p += 1
        out.append(p)
    return out
