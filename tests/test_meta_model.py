"""tests/meta_model.py against first principles, the relations of tests/test_gpu_metamorphic.py on the reference (the CPU oracle; the
envelope cost on envelope_model.dp_literal), and the sensitivity of the two optimality checks."""
import itertools

import numpy as np
import pytest

import brute
import envelope_model as em
import meta_model as mm
import plaid_total_model as ptm
import sym_model as sm
import test_gpu_metamorphic as gm
from util import cp, sprand, suitesparse_shaped, banded

MODELS = gm.ALL + (cp.AffineHyperedgeCutModel(1, 0, 2, 1, 5),)


def small_patterns():
    rng = np.random.default_rng(0xC0FFEE)
    return [sprand(m, n, p, rng) for m, n, p in ((5, 7, 0.4), (12, 23, 0.2), (9, 33, 0.3), (30, 40, 0.1), (6, 16, 0.0), (1, 9, 0.7))]


# ---------------------------------------------------------------- the checkers against first principles
def test_counts_and_costs_equal_the_brute_tables():
    for A in small_patterns():
        NT, ST = brute.net_table(A), brute.selfnet_table(A)
        n, ix = A.n, mm.index(A)
        for p in range(n + 1):
            for r in range(p, n + 1):
                assert mm.nets(A, p + 1, r + 1) == NT[p, r] and mm.selfnets(A, p + 1, r + 1) == ST[p, r], (A, p, r)
                assert mm.pins(A, p + 1, r + 1) == A.colptr[r] - A.colptr[p]
        for mdl in MODELS:
            F = brute.cost_table(A, mdl, None, NT, ST)
            for p in range(n + 1):
                for r in range(p, n + 1):
                    assert np.array_equal(mm.left_costs(ix, mdl, p, r), F[p, p:r + 1]), (A, p, r, mdl._params())
                    assert np.array_equal(mm.right_costs(ix, mdl, p, r), F[p:r + 1, r]), (A, p, r, mdl._params())
            for p, r in ((0, n), (1, n - 1), (n // 2, n)):
                assert mm.part_cost(A, mdl, p + 1, r + 1) == F[p, r]
        for spl in ([1, n + 1], [1, 1, 3, 3, n, n + 1, n + 1], [1, 2, n // 2, n // 2, n + 1], list(range(1, n + 2))):
            assert mm.split_selfnets(A, spl).tolist() == [mm.selfnets(A, spl[k], spl[k + 1]) for k in range(len(spl) - 1)], (A, spl)
            assert mm.total(A, gm.HCUT, spl) == sum(int(brute.cost_table(A, gm.HCUT, None, NT, ST)[spl[k] - 1, spl[k + 1] - 1]) for k in range(len(spl) - 1))


def test_envelope_and_plaid_sweeps_equal_the_definitions():
    rng = np.random.default_rng(5)
    for A in small_patterns():
        n, ix = A.n, mm.index(A)
        D = em.span_table(A)
        Pi = cp.MapPartition(3, rng.integers(1, 4, A.m))
        for p in range(n + 1):
            for r in range(p, n + 1):
                assert mm.span(A, p + 1, r + 1) == D[p, r]
                for mdl, k in ((gm.ENV, None), (gm.PCUT, 2), (gm.PRIM, 2), (gm.PRIM, 3)):
                    want = [mm.part_cost(A, mdl, p + 1, t + 1, k, Pi) for t in range(p, r + 1)]
                    assert mm.left_costs(ix, mdl, p, r, k, Pi).tolist() == want, (A, p, r, type(mdl).__name__)
                    want = [mm.part_cost(A, mdl, t + 1, r + 1, k, Pi) for t in range(p, r + 1)]
                    assert mm.right_costs(ix, mdl, p, r, k, Pi).tolist() == want, (A, p, r, type(mdl).__name__)
        E = em.Env(A, gm.ENV)
        assert np.array_equal(np.triu(E.table(1)), np.triu(np.array([[mm.part_cost(A, gm.ENV, p + 1, r + 1) if p <= r else 0 for r in range(n + 1)]
                                                                     for p in range(n + 1)])))


def test_symmetric_kinds_equal_the_dense_tables():
    """part_cost (set operations) and both sweeps against sym_model's dense tables; mirror_both keeps every count"""
    rng = np.random.default_rng(11)
    models = gm.SYM + (cp.AffineSymmetricConnectivityModel(1.0, 0.5, 2.0, 3.0, 7.0), cp.AffineMonotonizedSymmetricConnectivityModel(3, 1, 2, 5, 0))
    for n, p in ((1, 0.5), (7, 0.4), (16, 0.0), (23, 0.2), (33, 0.1)):
        A = sprand(n, n, p, rng)
        T, ix = sm.Tables(A), mm.index(A)
        for p0 in range(n + 1):
            for r in range(p0, n + 1):
                assert mm.dianets(A, p0 + 1, r + 1) == T.get("dianet")[p0, r] and mm.selfpins(A, p0 + 1, r + 1) == T.get("selfpin")[p0, r]
        B = mm.mirror_both(A)
        for name in ("dianet", "selfpin", "net"):
            assert np.array_equal(sm.Tables(B).get(name), sm.Tables(A).get(name)[::-1, ::-1].T), name
        for mdl in models:
            F = sm.cost_table(T, mdl)
            for p0 in range(n + 1):
                for r in range(p0, n + 1):
                    assert np.array_equal(mm.left_costs(ix, mdl, p0, r), F[p0, p0:r + 1]), (A, p0, r, mdl._params())
                    assert np.array_equal(mm.right_costs(ix, mdl, p0, r), F[p0:r + 1, r]), (A, p0, r, mdl._params())
                    if (p0 + r) % 3 == 0:
                        assert mm.part_cost(A, mdl, p0 + 1, r + 1) == F[p0, r], (A, p0, r, mdl._params())


def test_plaid_pair_equals_the_dense_tables():
    """the secondary model and the primary model under a SplitPartition (with an empty part) and a MapPartition"""
    rng = np.random.default_rng(12)
    for m, n, p in ((5, 7, 0.4), (12, 23, 0.2), (30, 19, 0.1), (6, 16, 0.0)):
        A = sprand(m, n, p, rng)
        ix = mm.index(A)
        cut = np.sort(rng.integers(1, m + 2, 2))
        Phi = cp.SplitPartition(4, np.array([1, cut[0], cut[0], cut[1], m + 1], dtype=np.int64))
        Pi = cp.MapPartition(4, rng.integers(1, 5, m))
        S = ptm.Secondary(A, Phi)
        for P in (Phi, Pi):
            T = ptm.Primary(A, P)
            for mdl in (gm.PRIM, gm.PRIM_BAND):
                for k in (1, 2, 4):
                    F = T.table(mdl, k)
                    for p0 in range(n + 1):
                        for r in range(p0, n + 1):
                            assert np.array_equal(mm.left_costs(ix, mdl, p0, r, k, P), F[p0, p0:r + 1]), (A, p0, r, k)
                            assert np.array_equal(mm.right_costs(ix, mdl, p0, r, k, P), F[p0:r + 1, r]), (A, p0, r, k)
                            if (p0 + r) % 3 == 0:
                                assert mm.part_cost(A, mdl, p0 + 1, r + 1, k, P) == F[p0, r]
        for mdl in (gm.SECOND, cp.AffineSecondaryConnectivityModel(1.0, 2.0, 0.5, 3.0, 1.0)):
            for k in (1, 2, 3, 4):
                F = S.table(mdl, k)
                for p0 in range(n + 1):
                    for r in range(p0, n + 1):
                        assert np.array_equal(mm.left_costs(ix, mdl, p0, r, k, Phi), F[p0, p0:r + 1]), (A, p0, r, k)
                        assert np.array_equal(mm.right_costs(ix, mdl, p0, r, k, Phi), F[p0:r + 1, r]), (A, p0, r, k)
                        if (p0 + r) % 3 == 0:
                            assert mm.part_cost(A, mdl, p0 + 1, r + 1, k, Phi) == F[p0, r]


def test_transforms():
    rng = np.random.default_rng(1)
    A = sprand(12, 23, 0.2, rng)

    def dense(B):
        X = np.zeros((B.m, B.n), bool)
        for j in range(B.n):
            X[B.rowval[B.colptr[j] - 1:B.colptr[j + 1] - 1] - 1, j] = True
        return X
    D = dense(A)
    assert np.array_equal(dense(mm.mirror_columns(A)), D[:, ::-1]) and np.array_equal(dense(mm.reverse_rows(A)), D[::-1])
    assert np.array_equal(dense(mm.shift_rows(A, 4)), np.vstack([np.zeros((4, A.n), bool), D]))
    for extra in (0, 5):
        B, sigma = mm.relabel_rows(A, rng, extra, return_map=True)
        assert B.m == A.m + extra and np.array_equal(dense(B)[sigma], D) and dense(B).sum() == D.sum()
    for B in (mm.mirror_columns(A), mm.reverse_rows(A), mm.relabel_rows(A, rng, 3)):
        assert all(np.all(np.diff(B.rowval[B.colptr[j] - 1:B.colptr[j + 1] - 1]) > 0) for j in range(B.n))
    spl = np.array([1, 4, 4, 20, 24])
    assert mm.total(mm.mirror_columns(A), gm.HCUT, mm.mirror_split(spl, A.n)) == mm.total(A, gm.HCUT, spl)
    assert mm.scaled(gm.HCUT, 3)._params() == [0, 6, 3, 9, 3] and mm.shifted(gm.CONN_D, 2)._params() == [2.5, 0.25, 1.0, 3.0]


def all_splits(n):
    """every split of 1 .. n into non-empty parts"""
    for r in range(n):
        for cut in itertools.combinations(range(2, n + 1), r):
            yield [1, *cut, n + 1]


def test_greedy_and_optimum_equal_exhaustive_search():
    rng = np.random.default_rng(77)
    seen = 0
    for m, n, p in ((6, 8, 0.3), (9, 10, 0.25), (4, 9, 0.5), (10, 7, 0.2)):
        A = sprand(m, n, p, rng)
        for mdl in (gm.CONN_I, gm.HCUT, gm.WORK, gm.CONN_D, gm.ENV):
            step = gm.step_of(mdl)
            for w, budget in ((None, None), (4, None), (None, max(int(np.diff(A.colptr).max()), A.nnz // 2))):
                ok = lambda s: mm.structure_ok(A, s, w, budget)
                table = [(len(s) - 1, mm.bottleneck(A, mdl, s)) for s in all_splits(n) if ok(s)]
                for c in sorted({v for _, v in table} | {0, 1, 10 ** 6}):
                    want = min((k for k, v in table if v <= c), default=mm.INFEASIBLE)
                    assert mm.greedy_parts(A, mdl, c, w, budget) == want, (A, mdl._params(), c, w, budget)
                    if c > mdl.alpha and w is None and budget is None and mdl is not gm.ENV:
                        least = [(len(s) - 1, min(mm.part_costs(A, mdl, s))) for s in all_splits(n)]
                        assert mm.most_parts(A, mdl, c) == max((k for k, v in least if v >= c), default=0), (A, mdl._params(), c)
                for K in (1, 2, 3):
                    vals = [v for k, v in table if k <= K]
                    want = min(vals) if vals else None
                    got = mm.bottleneck_optimum(A, mdl, K, w, budget, step=step)
                    assert got == want, (A, mdl._params(), K, w, budget, got, want)
                    if want is not None:
                        assert mm.certified(A, mdl, K, want, w, budget, step=step) and not mm.certified(A, mdl, K, want + step, w, budget, step=step)
                        seen += 1
                    if w is None and budget is None and mdl is not gm.ENV:
                        want = max(min(mm.part_costs(A, mdl, s)) for s in all_splits(n) if len(s) - 1 == K)
                        assert mm.maxmin_optimum(A, mdl, K, step=step) == want, (A, mdl._params(), K)
    assert seen > 100


def test_pair_slack_equals_exhaustive_search():
    rng = np.random.default_rng(3)
    A = sprand(9, 14, 0.3, rng)
    Pi = cp.MapPartition(3, rng.integers(1, 4, A.m))
    for mdl in (gm.CONN_I, gm.HCUT, gm.CONN_D, gm.ENV, gm.PCUT, gm.PRIM):
        for w, budget in ((None, None), (8, None), (None, A.nnz // 2 + 3)):
            for spl in ([1, 5, 9, 15], [1, 1, 8, 15], [1, 7, 8, 15], [1, 8, 15, 15]):
                if not mm.structure_ok(A, spl, w, budget):
                    continue
                want = []
                for k in range(2):
                    alt = [mm.part_cost(A, mdl, spl[k], t, k + 1, Pi) + mm.part_cost(A, mdl, t, spl[k + 2], k + 2, Pi) for t in range(spl[k], spl[k + 2] + 1)
                           if mm.structure_ok(A, [1, spl[k], t, spl[k + 2], A.n + 1], w, budget)]
                    here = mm.part_cost(A, mdl, spl[k], spl[k + 1], k + 1, Pi) + mm.part_cost(A, mdl, spl[k + 1], spl[k + 2], k + 2, Pi)
                    want.append(here - min(alt))
                assert mm.pair_slack(A, mdl, spl, w, budget, Pi) == want, (type(mdl).__name__, w, budget, spl)


# ---------------------------------------------------------------- the relations hold for the reference
@pytest.fixture(scope="module")
def ref(orc):
    return gm.Lib(orc)


@pytest.fixture(scope="module")
def pats():
    return ((gm.Pat(suitesparse_shaped(1500, 8, 4), 1), 7), (gm.Pat(banded(1200, 6, 0.5, 5), 2), 16))


def on_reference(ref, pats, check, cases):
    for case in cases:
        for P, K in pats:
            for mdl in case.at_small + case.at_tiny:
                check(ref, case, P, K, mdl, gm.limit(P.A, K, case.con))


def test_reference_structure_relabelling_and_mirror(ref, pats):
    on_reference(ref, pats, gm.check_structure, gm.CASES)
    on_reference(ref, pats, gm.check_relabel, gm.CASES)
    on_reference(ref, pats, gm.check_mirror, [c for c in gm.CASES if c.exact])


def test_reference_scaling_and_shift(ref, pats):
    on_reference(ref, pats, gm.check_scaling, gm.DP)
    on_reference(ref, pats, gm.check_scaling_bisect, gm.BISECT)
    on_reference(ref, pats, gm.check_shift, [c for c in gm.CASES if c.splitter])


def test_reference_relaxation(ref, pats):
    for method in ("total", "total_chunker", "bottleneck"):
        for P, K in pats:
            for mdl in gm.BY_ID[method].at_small:
                gm.check_relaxation(ref, method, P, K, mdl, bound=True)


def test_reference_optimality(ref, pats):
    on_reference(ref, pats, gm.check_pair, [c for c in gm.DP if c.objective == "sum"])
    on_reference(ref, pats, gm.check_certificate, gm.CERTIFIED)
    on_reference(ref, pats, gm.check_within_eps, gm.APPROX)


def test_reference_plaid_connectivity(ref, pats):
    for P, K in pats:
        gm.check_plaid(ref, gm.PLAID_CASES[1], P, K, gm.PRIM)


def test_reference_plaid_pair_total(ref):
    """the relations of the primary and the secondary total on the reference, with their optima of many parts"""
    for name, P, K in (("ss", gm.Pat(suitesparse_shaped(1500, 8, 4), 1), 7), ("band", gm.Pat(banded(1200, 6, 0.5, 5), 2), 16)):
        for mdl in (gm.PRIM, gm.PRIM_BAND):
            gm.check_primary(ref, gm.PRIMARY_CASE, P, K, mdl, name)
        gm.check_secondary(ref, gm.SECONDARY_CASE, P, K, gm.SECOND, name)


class EnvLiteral:
    """the literal K-layer DP of tests/envelope_model.py in the place of the library"""

    def __call__(self, A, K, method, mdl, con=None, Pi=None, engine=None):
        return em.dp_literal(em.Env(A, mdl), K, "sum" if method == "total" else "max")[0]

    def base(self, A, K, case, mdl, con, Pi=None):
        return self(A, K, case.method, mdl)


@pytest.mark.parametrize("case", gm.ENV_CASES, ids=gm.ids(gm.ENV_CASES))
def test_reference_envelope(case):
    for P, K in ((gm.Pat(banded(300, 6, 0.5, 8), 3), 7), (gm.Pat(suitesparse_shaped(257, 6, 9), 4), 5)):
        gm.check_envelope(EnvLiteral(), case, P, K)


# ---------------------------------------------------------------- sensitivity
def test_pair_optimal_flags_exactly_the_moves_that_raise_the_total(ref, pats):
    raised = kept = 0
    for P, K in pats:
        A = P.A
        for mdl in (gm.CONN_I, gm.CONN_F):
            con = gm.limit(A, K, "w15")
            spl = ref.base(A, K, gm.BY_ID["total-w15"], mdl, con)
            best = mm.total(A, mdl, spl)
            assert mm.pair_optimal(A, mdl, spl, **gm.kw(con))
            for k in range(1, K):
                for d in (-7, -1, 1, 7):
                    moved = spl.copy(); moved[k] += d
                    if not mm.structure_ok(A, moved, **gm.kw(con)):
                        continue
                    worse = mm.total(A, mdl, moved) > best
                    assert mm.pair_optimal(A, mdl, moved, **gm.kw(con)) == (not worse), (K, k, d, spl)
                    raised += worse; kept += not worse
    assert raised > 50, (raised, kept)


def test_certificate_rejects_a_split_whose_bottleneck_rose(ref, pats):
    rejected = 0
    for P, K in pats:
        A = P.A
        for mdl, kind in ((gm.CONN_I, None), (gm.HCUT, "w15"), (gm.WORK, "pins"), (gm.CONN_D, None)):
            con = gm.limit(A, K, kind)
            spl = ref.base(A, K, gm.BY_ID["bottleneck" if kind is None else f"bottleneck-{kind}"], mdl, con)
            best = mm.bottleneck(A, mdl, spl)
            assert mm.certified(A, mdl, K, best, step=gm.step_of(mdl), **gm.kw(con))
            for k in range(1, K):
                for d in (-7, 7):
                    moved = spl.copy(); moved[k] += d
                    if mm.structure_ok(A, moved, **gm.kw(con)) and mm.bottleneck(A, mdl, moved) > best:
                        assert not mm.certified(A, mdl, K, mm.bottleneck(A, mdl, moved), step=gm.step_of(mdl), **gm.kw(con))
                        rejected += 1
    assert rejected > 20, rejected
