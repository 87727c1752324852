"""The total-cost DP of the envelope model by divide and conquer over the cut column, restated in Python as the device runs it
(csrc/envelope_total.hip): the candidate key V and the row term Rw, the leaf pass over aligned blocks of `leaf` rows, and per
level h = leaf, 2 leaf, ... <= n the three derived keys, the two binary searches per row and the four regimes.  Every minimum is a
query of the same two-level range-minimum structure the device builds -- blocks of `leaf` entries with an in-block table of
offsets, a sparse table of positions over the block minima -- and returns its rightmost argument.

Indices are 0-based here (r = j' - 1, a = j - 1); the tables come back as envelope_model.dp_literal returns them."""
import numpy as np

import envelope_model as em


def dc_ok(mdl, m, n, N, K):
    """env_dc_ok: no condition on the sign of a beta; the bound K max|alpha| + n |b_vertex| + N |b_pin| + K m |b_net| (a total
    sums up to K parts, so the net term enters K times) below 2^60 for Int64, below 2^51 with finite integral parameters for Float64"""
    ak = list(getattr(mdl, "alpha_k", None) or [])
    params = [mdl.alpha, mdl.beta_vertex, mdl.beta_pin, mdl.beta_net] + ak
    if not em.is_int_model(mdl):
        if not all(np.isfinite(v) and float(v).is_integer() and abs(v) < 2.0 ** 51 for v in params):
            return False
    k = max(K, 1)
    amax = max(abs(int(v)) for v in [mdl.alpha] + ak)
    bound = amax * k + abs(int(mdl.beta_vertex)) * n + abs(int(mdl.beta_pin)) * N + abs(int(mdl.beta_net)) * m * k
    return bound < (2 ** 60 if em.is_int_model(mdl) else 2 ** 51)


class Rmq:
    """rightmost minimum of key over [x, y]: blocks of B = 2^T entries (len(key) is a multiple of B)"""

    def __init__(self, key, B):
        assert B >= 2 and B & (B - 1) == 0 and len(key) % B == 0
        self.key, self.B, self.T = key, B, B.bit_length() - 1
        n = len(key)
        lane = np.arange(n) % B
        v, off = key.copy(), np.zeros(n, dtype=np.int64)
        self.ib = [off.copy()]
        for t in range(1, self.T + 1):                         # after step t: the rightmost minimum of [a, a + 2^t) cut at the block's end
            sh = 1 << (t - 1)
            pv, po = np.roll(v, -sh), np.roll(off, -sh)
            take = (lane + sh < B) & (pv <= v)                 # (the partner's window lies to the right: it wins ties)
            v, off = np.where(take, pv, v), np.where(take, po + sh, off)
            self.ib.append(off.copy())
        nb = n // B
        self.bt = [np.arange(nb, dtype=np.int64) * B + off[::B]]
        s = 1
        while (1 << s) <= nb:
            below, cur = self.bt[-1], self.bt[-1].copy()
            for b in range(nb):
                b2 = b + (1 << (s - 1))
                if b2 < nb and key[below[b2]] <= key[below[b]]:
                    cur[b] = below[b2]
            self.bt.append(cur)
            s += 1

    def _block(self, x, y):
        t = (y - x + 1).bit_length() - 1
        if t == 0:
            return x
        x2 = y - (1 << t) + 1
        i1, i2 = x + int(self.ib[t][x]), x2 + int(self.ib[t][x2])
        return i2 if self.key[i2] <= self.key[i1] else i1

    def query(self, x, y):
        assert 0 <= x <= y < len(self.key)
        B, key = self.B, self.key
        bx, by = x // B, y // B
        if bx == by:
            return self._block(x, y)
        i = self._block(x, bx * B + B - 1)
        if by > bx + 1:
            s = (by - bx - 1).bit_length() - 1
            j1, j2 = int(self.bt[s][bx + 1]), int(self.bt[s][by - (1 << s)])
            j = j2 if key[j2] <= key[j1] else j1
            if key[j] <= key[i]:
                i = j
        j = self._block(by * B, y)
        return j if key[j] <= key[i] else i


def _layer(E, k, W, leaf, counts):
    """all rows of layer k from the previous layer's costs W -> (cst, ptr 0-based)"""
    A, dt = E.A, E.dt
    n, m = A.n, A.m
    n1 = n + 1
    bv, bp, bn = dt(E.mdl.beta_vertex), dt(E.mdl.beta_pin), dt(E.mdl.beta_net)
    idx, pos = np.arange(n1, dtype=np.int64), E.pos - 1
    V = (W - idx.astype(dt) * bv) - pos.astype(dt) * bp
    Rw = (E.alpha(k) + idx.astype(dt) * bv) + pos.astype(dt) * bp
    lo_leaf, hi_leaf = E.lo, E.hi

    def lohi(p, r):                                            # the leaves [p, r), p < r <= n
        return int(lo_leaf[p:r].min()), int(hi_leaf[p:r].max())

    n1p = -(-n1 // leaf) * leaf
    key0 = np.zeros(n1p, dtype=dt)
    key0[:n1] = V
    R0 = Rmq(key0, leaf)
    cst, ptr = np.zeros(n1, dtype=dt), np.zeros(n1, dtype=np.int64)
    for r in range(n1):                                        # the leaf pass: the pairs inside the block and the diagonal
        lo, hi, best, arg = m + 1, 0, None, -1
        for p in range(r, r - r % leaf - 1, -1):
            if p < r:
                lo, hi = min(lo, int(lo_leaf[p])), max(hi, int(hi_leaf[p]))
            v = V[p] + dt(max(hi - lo, 0)) * bn
            if best is None or v < best:
                best, arg = v, p
        cst[r], ptr[r] = best + Rw[r], arg
    h = leaf
    while h <= n:
        keys = [key0.copy() for _ in range(3)]
        for a in range(n1p):
            half = a // h
            mid = (half + 1) * h
            if half % 2 == 0 and mid <= n:
                sl, sh = lohi(a, mid)
                keys[0][a] = key0[a] + dt(max(sh - sl, 0)) * bn
                keys[1][a] = key0[a] + dt(sh) * bn
                keys[2][a] = key0[a] - dt(sl) * bn
        R1, R2, R3 = (Rmq(kk, leaf) for kk in keys)
        cnt = counts.setdefault(h, [0, 0, 0, 0]) if counts is not None else [0, 0, 0, 0]
        for mid in range(h, n1, 2 * h):
            L = mid - h
            for r in range(mid, min(mid + h, n1)):
                PL, PH = lohi(mid, r) if r > mid else (m + 1, 0)
                lo, hi = 0, h
                while lo < hi:
                    x = (lo + hi) >> 1
                    if lohi(L + x, mid)[1] >= PH:
                        lo = x + 1
                    else:
                        hi = x
                xa = lo
                lo, hi = 0, h
                while lo < hi:
                    x = (lo + hi) >> 1
                    if lohi(L + x, mid)[0] <= PL:
                        lo = x + 1
                    else:
                        hi = x
                xb = lo
                x0, x1 = min(xa, xb), max(xa, xb)
                best, arg = cst[r], int(ptr[r])

                def take(key, a):
                    nonlocal best, arg
                    v = key + Rw[r]
                    if v < best or (v == best and a > arg):
                        best, arg = v, a
                if x0 > 0:
                    a = R1.query(L, L + x0 - 1)
                    take(keys[0][a], a); cnt[0] += x0
                if x1 < h:
                    a = R0.query(L + x1, mid - 1)
                    take(key0[a] + dt(max(PH - PL, 0)) * bn, a); cnt[1] += h - x1
                if x0 < x1:
                    if xa > xb:
                        a = R2.query(L + x0, L + x1 - 1)
                        take(keys[1][a] - dt(PL) * bn, a); cnt[2] += x1 - x0
                    else:
                        a = R3.query(L + x0, L + x1 - 1)
                        take(keys[2][a] + dt(PH) * bn, a); cnt[3] += x1 - x0
                cst[r], ptr[r] = best, arg
        h *= 2
    return cst, ptr


def dp_dc(E, K, leaf=64, counts=None):
    """the K-part total DP -> (spl, cst, ptr) as em.dp_literal(E, K, "sum") returns them.  A layer of one row (layer K; n = 0) is
    a single reduction over the candidates in the reference's order.  counts: {h: pairs per regime} summed over the layers"""
    n = E.A.n
    cst = np.full((n + 1, K), em._typemax(E), dtype=E.dt)
    ptr = np.zeros((n + 1, K), dtype=np.int64)
    cst[:, 0] = E.row(1, 1)
    ptr[:, 0] = 1
    with np.errstate(over="ignore"):
        for k in range(2, K + 1):
            W = cst[:, k - 2]
            if k == K or n == 0:
                v = W + E.column(n + 1, k)
                i = v.size - 1 - int(np.argmin(v[::-1]))
                cst[n, k - 1], ptr[n, k - 1] = v[i], i + 1
            else:
                c, p = _layer(E, k, W, leaf, counts)
                cst[:, k - 1], ptr[:, k - 1] = c, p + 1
    return em.unravel(K, n, ptr), cst, ptr


def regime_counts(E, K, leaf=64):
    """{h: [pairs with both extrema from the candidate side, both from the row side, hi from the candidate and lo from the row,
    lo from the candidate and hi from the row]} over the upper levels of every full layer"""
    counts = {}
    dp_dc(E, K, leaf, counts)
    return counts
