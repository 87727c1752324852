"""GPU tests of the total-cost DP of the envelope model by divide and conquer (csrc/envelope_total.hip): every table cell against
the literal DP and against the device sweep, the gates, a size past the sweep's reach at default options, and the permuting and
alternating callers.

Shapes: DP rows n + 1 in 1, 2, 3 (one-row layers and one lane), 64 and 65 (one leaf block and one row past it), 128 and 129 (a top
node whose right half is a single row), 257 (a truncated last node); n in 1025, 5000 (more than one workgroup and more than one
level of the table over block minima); n = 200 001 where the sweep is refused."""
import functools

import numpy as np
import pytest

import envelope_dc_model as dc
import envelope_model as em
from test_gpu_envelope import _from_dense, option, pattern, tables
from util import banded, cp, golden_matrices, suitesparse_shaped

pytestmark = pytest.mark.gpu
ENV = cp.AffineEnvelopeModel
SUM = 0
MIN_N = 256                                                    # the default of env_dc_min_n (csrc/envelope_total.hip)


def dc_layers(hip, call):
    hip.set_option("stat_reset", 0)
    out = call()
    return out, hip.get_stat("env_dc_layers")


def models(K):
    ak = [int(v) for v in np.random.default_rng(K).integers(-3, 6, K)]
    return [ENV(0, 10, 1, 100), ENV(1, 1, 2, 3, alpha_k=ak), ENV(0, 0, 0, 0), ENV(0, 1, -1, 2), ENV(3, -2, 1, -1), ENV(0.0, 10.0, 1.0, 100.0)]


@functools.lru_cache(maxsize=None)
def cell_pattern(name):
    if name == "empty":                                        # no entry at all: every span is 0
        return cp.SparseMatrixCSC(50, 128, np.ones(129, dtype=np.int64), np.zeros(0, dtype=np.int64))
    if name == "m1":
        return _from_dense(np.random.default_rng(5).random((1, 256)) < 0.4)
    n = int(name)
    seed = {127: 301, 128: 316, 256: 301}.get(n, 300 + n)      # (seeds whose upper levels hold all four regimes, see the next test)
    return pattern(50, n, seed, dens=0.1, full=n > 0)


# ---------------------------------------------------------------- every cell against the literal DP
def test_inputs_reach_all_four_regimes():
    """a condition on the inputs of the next test, checked on the CPU model: every random pattern with an upper level that has more
    than one row reaches the four regimes there"""
    for name in ("127", "128", "256"):
        counts = dc.regime_counts(em.Env(cell_pattern(name), ENV(0, 10, 1, 100)), 3, 64)
        assert counts and all(c > 0 for c in np.sum(list(counts.values()), axis=0)), (name, counts)


@pytest.mark.parametrize("name", ["0", "1", "2", "63", "64", "127", "128", "256", "empty", "m1"])
def test_every_cell_matches_the_literal_dp(hip, name):
    A = cell_pattern(name)
    n = A.n
    with option(hip, "env_dc_min_n", 0, MIN_N):
        for K in (1, 2, 5, n + 3):
            for mdl in models(K):
                spl, cst, ptr = em.dp_literal(em.Env(A, mdl), K, "sum")
                (gp, gc), layers = dc_layers(hip, lambda: tables(hip, A, K, SUM, mdl))
                assert layers == K - 1, (name, K, mdl._params())
                assert np.array_equal(gp, ptr) and np.array_equal(gc, cst), (name, K, mdl._params())
                assert np.array_equal(cp.partition_stripe(A, K, cp.DynamicTotalSplitter(mdl), backend=hip).spl, spl)
                if mdl._params() == ENV(0, 0, 0, 0)._params() and K > 2:      # every candidate ties: the diagonal wins
                    assert np.array_equal(gp[:, 1], np.arange(1, n + 2))
            assert np.array_equal(cp.partition_stripe(A, K, cp.ReferenceTotalSplitter(models(K)[0]), backend=hip).spl,
                                  em.dp_literal(em.Env(A, models(K)[0]), K, "sum")[0])


# ---------------------------------------------------------------- the gates
def test_gates(hip):
    A = pattern(50, 64, 364, dens=0.1)
    with option(hip, "env_dc_min_n", 0, MIN_N):
        for mdl, K, want in ((ENV(0.5, 0.25, 0.1, 1.7), 4, 0), (ENV(2 ** 58, 1, 1, 1), 4, 0), (ENV(2 ** 58, 1, 1, 1), 3, 2)):
            (gp, gc), layers = dc_layers(hip, lambda: tables(hip, A, K, SUM, mdl))
            _, cst, ptr = em.dp_literal(em.Env(A, mdl), K, "sum")
            assert layers == want and np.array_equal(gp, ptr) and np.array_equal(gc, cst), (mdl._params(), K)
        with option(hip, "force_brute", 1, 0):
            (gp, gc), layers = dc_layers(hip, lambda: tables(hip, A, 4, SUM, ENV(0, 10, 1, 100)))
        assert layers == 0
        (gp2, gc2), layers = dc_layers(hip, lambda: tables(hip, A, 4, SUM, ENV(0, 10, 1, 100)))
        assert layers == 3 and np.array_equal(gp, gp2) and np.array_equal(gc, gc2)
    B = pattern(40, 300, 6, dens=0.1)
    ok, frac = ENV(0, 10, 1, 100), ENV(0.5, 0.25, 0.1, 1.7)
    with option(hip, "brute_max_n", 100, 200000):
        with option(hip, "env_dc_min_n", 0, MIN_N):
            got, layers = dc_layers(hip, lambda: cp.partition_stripe(B, 3, cp.DynamicTotalSplitter(ok), backend=hip).spl)
            assert layers == 2 and np.array_equal(got, em.dp_literal(em.Env(B, ok), 3, "sum")[0])
            with pytest.raises(NotImplementedError, match="AffineEnvelopeModel"):
                cp.partition_stripe(B, 3, cp.DynamicTotalSplitter(frac), backend=hip)
        with option(hip, "env_dc_min_n", 10 ** 9, MIN_N):
            with pytest.raises(NotImplementedError, match="AffineEnvelopeModel"):
                cp.partition_stripe(B, 3, cp.DynamicTotalSplitter(ok), backend=hip)


# ---------------------------------------------------------------- past one workgroup and one range-minimum block
@pytest.mark.parametrize("n", [1025, 5000])
def test_every_cell_matches_the_device_sweep(hip, n):
    K = 4
    for A in (suitesparse_shaped(n, 6, 50 + n), banded(n, 20, 0.3, 60 + n)):
        for mdl in (ENV(0, 10, 1, 100), ENV(0, 1, -1, 2), ENV(2.0, 3.0, 1.0, 7.0)):
            with option(hip, "env_dc_min_n", 0, MIN_N):
                (gp, gc), layers = dc_layers(hip, lambda: tables(hip, A, K, SUM, mdl))
            assert layers == K - 1
            with option(hip, "force_brute", 1, 0):
                (bp, bc), layers = dc_layers(hip, lambda: tables(hip, A, K, SUM, mdl))
            assert layers == 0
            assert np.array_equal(gp, bp) and np.array_equal(gc, bc), (n, mdl._params())


# ---------------------------------------------------------------- past the sweep's reach at default options
@pytest.mark.parametrize("mdl", [ENV(0, 10, 1, 100), ENV(0, 1, -1, 2)], ids=["pos", "neg"])
def test_past_the_sweep_at_default_options(hip, mdl):
    n, K = 200_001, 3
    A = suitesparse_shaped(n, 6, 43)
    Phi = cp.partition_stripe(A, K, cp.DynamicTotalSplitter(mdl), backend=hip)      # (NotImplementedError without the divide and conquer)
    (ptr, cst), layers = dc_layers(hip, lambda: tables(hip, A, K, SUM, mdl))
    assert layers == 2
    E = em.Env(A, mdl, tables=False)
    rng = np.random.default_rng(44)
    cells = [(K, n + 1)] + [(2, int(rng.integers(1, n + 2))) for _ in range(64)]
    for k, jp in cells:
        with np.errstate(over="ignore"):
            v = cst[:jp, k - 2] + E.column(jp, k)
        i = v.size - 1 - int(np.argmin(v[::-1]))
        assert cst[jp - 1, k - 1] == v[i] and ptr[jp - 1, k - 1] == i + 1, (k, jp)
    assert np.array_equal(ptr[:, 0], np.ones(n + 1, dtype=np.int64)) and np.array_equal(cst[:, 0], E.row(1, 1))
    assert np.array_equal(Phi.spl, em.unravel(K, n, ptr))
    assert cp.total_value(A, Phi, mdl, backend=hip) == cst[n, K - 1]


# ---------------------------------------------------------------- callers
def test_permuting_and_alternating_callers(hip):
    mdl = ENV(0, 10, 1, 100)
    A = golden_matrices()["HB/can_292"]
    B = pattern(120, 300, 7, dens=0.05)
    perm = cp.PermutingPartitioner(cp.CuthillMcKeePermuter(), cp.DynamicTotalSplitter(mdl))
    alt = cp.AlternatingPartitioner(cp.DynamicBottleneckSplitter(mdl), cp.DynamicTotalSplitter(mdl), cp.DynamicTotalSplitter(mdl))

    def run():
        return cp.partition_stripe(A, 4, perm, backend=hip), cp.partition_plaid(B, 4, alt, backend=hip)

    with option(hip, "env_dc_min_n", 0, MIN_N):
        (dom, (Pi, Phi)), layers = dc_layers(hip, run)
    assert layers == 3 * 3
    with option(hip, "force_brute", 1, 0):
        (dom_b, (Pi_b, Phi_b)), layers = dc_layers(hip, run)
    assert layers == 0
    assert isinstance(dom, cp.DomainPartition) and dom == dom_b
    assert np.array_equal(Pi.spl, Pi_b.spl) and np.array_equal(Phi.spl, Phi_b.spl)
