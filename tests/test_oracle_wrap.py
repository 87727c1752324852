"""Pins the oracle as the arbiter for Int64 costs that WRAP (Julia's Int64 arithmetic: two's complement, no error).

A model such as AffineConnectivityModel(0, 1, 1, 3*2^61) overflows on every part with a net; the reference then computes its
recurrence on the wrapped values.  The oracle must reproduce that literally -- every cell of cst / ptr equal to brute force
(tests/brute.py: counts from their definitions, the recurrence as written) evaluated in wrapped numpy int64 -- because the GPU
tests of the same models (test_gpu_value_edges.py) take the oracle as ground truth."""
import numpy as np
import pytest

import brute
from util import cp, sprand, golden_matrices

WRAP = [cp.AffineConnectivityModel(0, 1, 1, 3 * 2 ** 61), cp.AffineConnectivityModel(0, 1, 1, 2 ** 62 + 99),
        cp.AffineConnectivityModel(0, 1, 1, 2 ** 61 + 7), cp.AffineWorkModel(0, 1, 2 ** 62 + 1),
        cp.AffineHyperedgeCutModel(0, 1, 1, 2 ** 62 + 5, 2 ** 61 + 3),
        cp.AffineConnectivityModel(0, 1, 1, 5, alpha_k=[2 ** 62, -2 ** 62, 3, 2 ** 62 + 1, -2 ** 62 - 7])]


def mats():
    rng = np.random.default_rng(0x5EED)
    out = [sprand(m, n, p, rng) for (m, n, p) in [(3, 2, 0.5), (5, 7, 0.4), (8, 16, 0.3), (12, 24, 0.3), (10, 23, 0.2)]]
    return out + [golden_matrices()["LPnetlib/lpi_itest6"]]


def wrapped_layer(W, F, g, lo=None, hi=None):
    """brute.layer for g = min-sum or min-max, in int64 (the sum wraps, as the reference's does)"""
    if g == 0:
        return brute.layer(W, F, lo, hi)
    n1 = F.shape[0]
    cst = np.zeros(n1, dtype=np.int64); ptr = np.full(n1, -1, dtype=np.int64)
    for r in range(n1):
        a = 0 if lo is None else int(lo[r])
        b = r if hi is None else int(hi[r])
        if b < a:
            continue
        v = np.maximum(W[a:b + 1], F[a:b + 1, r])
        i = v.size - 1 - int(np.argmin(v[::-1]))
        cst[r] = v[i]; ptr[r] = a + i
    return cst, ptr


@pytest.mark.parametrize("g", [0, 1])
def test_unconstrained_tables_under_wrap(orc, g):
    """every cell of layers 1 .. K-1 and the last layer's only cell (j' = n+1), sum and max; the sum optimum also equals
    the wrapped K-fold recurrence started from scratch"""
    with np.errstate(over="ignore"):
        for A in mats():
            n = A.n
            NT, ST = brute.net_table(A), brute.selfnet_table(A)
            for mdl in WRAP:
                K = 5
                rc, ptr, cst = orc.dynamic_tables(A, K, g, mdl.marshal(), None)
                assert rc == 0
                F1 = brute.cost_table(A, mdl, 1, NT, ST)
                assert np.array_equal(cst[:, 0], F1[0, :]) and np.all(ptr[:, 0] == 1)
                W = F1[0, :].copy()
                for k in range(2, K + 1):
                    F = brute.cost_table(A, mdl, k, NT, ST)
                    c2, p2 = wrapped_layer(W, F, g)
                    rows = slice(None) if k < K else slice(n, n + 1)
                    assert np.array_equal(c2[rows], cst[rows, k - 1]), (A, mdl.kind, k)
                    assert np.array_equal(p2[rows] + 1, ptr[rows, k - 1]), (A, mdl.kind, k)
                    W = c2
                if g == 0:
                    spl = cp.partition_stripe(A, K, cp.DynamicTotalSplitter(mdl), backend=orc)
                    assert cp.total_value(A, spl, mdl, backend=orc) == int(W[n])


def test_wrapped_costs_are_outside_the_fast_class():
    """the premise of the gate: the fast layers assume inverse-Monge costs, whose largest arg-mins never decrease along a row;
    with a wrapped b_net brute force breaks that on some layers, with a small b_net on none -- so the fast paths must refuse
    such models"""
    rng = np.random.default_rng(40)
    differ = {}
    with np.errstate(over="ignore"):
        for b in (3 * 2 ** 61, 2 ** 62 + 99, 100):
            mdl = cp.AffineConnectivityModel(0, 1, 1, b)
            differ[b] = 0
            for _ in range(12):
                A = sprand(12, 24, 0.3, rng)
                F = brute.cost_table(A, mdl)
                W = F[0, :].copy()
                _, pb = brute.layer(W, F)
                # inverse-Monge rows have non-decreasing largest arg-mins; a wrapped cost breaks that
                differ[b] += int(np.any(np.diff(pb) < 0))
    assert differ[100] == 0
    assert differ[3 * 2 ** 61] > 0 and differ[2 ** 62 + 99] > 0


@pytest.mark.parametrize("g", [0, 1])
def test_windowed_tables_under_wrap(orc, g):
    """ConstrainedCost(f, VertexCount(), w): every in-window cell of every layer equals the wrapped brute-force recurrence
    over the candidates max(lo[k-1], j'-w) <= j <= min(j', hi[k-1]) (DynamicSplitter.jl:233-246)"""
    nondeg = 0
    with np.errstate(over="ignore"):
        for A in mats():
            n = A.n
            NT, ST = brute.net_table(A), brute.selfnet_table(A)
            for mdl in WRAP:
                for K in (2, 3, 5):
                    for w in sorted({max(1, -(-n // K)), max(1, -(-3 * n // (2 * K))), n}):
                        rc, lo, hi, ptr, cst = orc.dynamic_tables_constrained(A, K, g, mdl.marshal(), None, cp.VertexCount().marshal(), w, float(w))
                        if rc == 2:
                            continue
                        assert rc == 0
                        a0, b0 = lo[0] - 1, hi[0] - 1
                        F1 = brute.cost_table(A, mdl, 1, NT, ST)
                        assert np.array_equal(cst[a0:b0 + 1, 0], F1[0, a0:b0 + 1])
                        W = cst[:, 0].copy()
                        for k in range(2, K + 1):
                            F = brute.cost_table(A, mdl, k, NT, ST)
                            r = np.arange(n + 1)
                            clo = np.maximum(lo[k - 2] - 1, r - w); chi = np.minimum(r, hi[k - 2] - 1)
                            c2, p2 = wrapped_layer(W, F, g, clo, chi)
                            a, b = lo[k - 1] - 1, hi[k - 1] - 1
                            assert np.array_equal(p2[a:b + 1] + 1, ptr[a:b + 1, k - 1]), (A, mdl.kind, K, w, k)
                            assert np.array_equal(c2[a:b + 1], cst[a:b + 1, k - 1]), (A, mdl.kind, K, w, k)
                            W = cst[:, k - 1].copy()
                        want = cp.partition_stripe(A, K, (cp.DynamicTotalSplitter if g == 0 else cp.DynamicBottleneckSplitter)(
                            cp.ConstrainedCost(mdl, cp.VertexCount(), w)), backend=orc)
                        nondeg += int(len(set(want.spl.tolist())) > 2)
    assert nondeg > 20
