"""Optimality and invariance of the split vectors past the CPU oracle's reach, refereed by tests/meta_model.py alone: values from the
definitions, exact host certificates and exact invariances of the problem.  No oracle, no second opinion of the library's own.

Sizes: n = 4 099 (just past 2^12, no multiple of 64 or 256) and n = 70 001 (17 bit planes, 274 column blocks).  At n = 70 001 every call
runs with brute_max_n = 0, so an O(n^2) sweep is refused rather than taken, and the first call of a case reads the profile slots and
stats as tests/test_gpu_dp_routing.py does and asserts that the case's engine ran.  A (model, constraint) pair that the library
serves by a sweep runs at n = 4 099 only; a pair it serves by the one-wave literal kernel (a total cost outside the inverse-Monge
gate, or a Float64 bottleneck, under a ConstrainedCost or in pack_stripe) runs every relation at n = 1 031 on one pattern and K: that
kernel is Theta(n w) steps of one wave.

The symmetric cost family (SymTotal) and the plaid connectivity pair (PlaidTotal for the primary model, PlaidScan for the secondary)
run the relations of the total objective at both sizes; at n = 70 001 their engines are asserted like the others.  Inside SymTotal's
gate a symmetric cost is alpha plus a subadditive function of the range, so its total optimum is the closed form [1, n + 1, ...] like
the unconstrained connectivity total: those cases take part in the identities and in pair_slack == 0, and it is the plaid pair that
brings optima with many parts in use (asserted).

All model parameters are integers or dyadic rationals and all sums stay far below 2^53: every comparison is `==`.

The relations are written over a solver `lib(A, K, method, mdl, con, Pi)`, so tests/test_meta_model.py runs the same code on the
CPU oracle at sizes the oracle reaches."""
import contextlib
import functools
import math
from collections import namedtuple

import numpy as np
import pytest

import meta_model as mm
from util import cp, suitesparse_shaped, banded

pytestmark = pytest.mark.gpu

TINY, SMALL, SCALE, REDUCED = 1031, 4099, 70001, 20001
EPS = 0.01
CONN_I = cp.AffineConnectivityModel(0, 10, 1, 100)
HCUT = cp.AffineHyperedgeCutModel(0, 2, 1, 3, 1)                     # grows with its part (self >= cut): the bottleneck engines take it
HCUT_M = cp.AffineHyperedgeCutModel(0, 2, 1, 1, 3)                   # self <= cut: the hyperedge form the scalable total-cost engines take
WORK = cp.AffineWorkModel(0, 10, 1)
CONN_F = cp.AffineConnectivityModel(0.0, 3.0, 1.0, 7.0)              # integral Float64
CONN_D = cp.AffineConnectivityModel(0.5, 0.25, 1.0, 3.0)             # dyadic Float64: every cost a multiple of 1/4
ENV = cp.AffineEnvelopeModel(0, 10, 1, 100)
ENV_SPREAD = cp.AffineEnvelopeModel(0, 10, 1, -3)
PCUT = cp.AffinePrimaryEdgeCutModel(0, 2, 1, 7)
PRIM = cp.AffinePrimaryConnectivityModel(0, 2, 1, 1, 7)
PINS = cp.AffineWorkModel(0, 0, 1)
SYM = (cp.AffineSymmetricConnectivityModel(0, 2, 1, 1, 7), cp.AffineMonotonizedSymmetricConnectivityModel(0, 0, 1, 100, 2),
       cp.AffineSymmetricEdgeCutModel(0, 2, 1, 7))
PRIM_BAND = cp.AffinePrimaryConnectivityModel(0, 2, 1, 0, 100)      # remote far above local: under banded owners every part follows its rows
SECOND = cp.AffineSecondaryConnectivityModel(0, 2, 1, 1, 7)
MONGE = (CONN_I, WORK, CONN_F, HCUT_M)                               # the scalable total-cost engines (and the LWS chunker) take these
INT = (CONN_I, WORK, HCUT)                                           # the constrained valley search takes Int64 costs only
ALL = (CONN_I, WORK, HCUT, CONN_F, CONN_D)
# The models outside those gates are served under a ConstrainedCost by the one-wave literal kernel, Theta(n w) steps of a single
# wave, and in pack_stripe likewise: they run every relation at n = TINY on one pattern and K, where a call takes about a second.
ONE_WAVE_TOTAL = (HCUT, CONN_D)
ONE_WAVE_BOTTLENECK = (CONN_F, CONN_D)
# LazyBisectCost has a connectivity specialisation only: the library and the oracle refuse a Work or hyperedge model ("violated precondition").
CONN = (CONN_I, CONN_F, CONN_D)
# BisectCost and BisectIndex have no hyperedge form (CP_EUNSUPPORTED on the device and on the oracle).  Under a factor of 2^20 the split
# of BisectIndex is identical, that of the cost bisections is not, on the reference itself: their bounds hold alpha + floor(s / K), which a
# factor moves by a fraction of a unit (oracle, banded(1200, 6, 0.5, 5), K = 16: BisectCost differs in 14 boundaries with
# AffineWorkModel(0, 10, 1), BisectCost and LazyBisectCost in 11 with the integral Float64 model) -- see check_scaling_bisect.
BISECTED = (CONN_I, WORK, CONN_F, CONN_D)

METHODS = {"total": cp.DynamicTotalSplitter, "total_chunker": cp.DynamicTotalChunker, "bottleneck": cp.DynamicBottleneckSplitter,
           "bisect_index": cp.BisectIndexBottleneckSplitter, "bisect_cost": lambda f: cp.BisectCostBottleneckSplitter(f, EPS),
           "lazy": lambda f: cp.LazyBisectCostBottleneckSplitter(f, EPS), "lazy_flip": lambda f: cp.LazyFlipBisectCostBottleneckSplitter(f, EPS)}
PACK = {"pack_dynamic": cp.DynamicTotalChunker, "pack_convex": cp.ConvexTotalChunker}


def step_of(mdl):
    return 0.25 if mdl is CONN_D else 1


def key_of(mdl):
    return (type(mdl).__name__, tuple(mdl._params()))


# ---------------------------------------------------------------- patterns
def _from_entries(m, n, c, r):
    key = np.unique(c.astype(np.int64) * (m + 1) + r.astype(np.int64))
    c, r = key // (m + 1), key % (m + 1)
    colptr = np.concatenate([[1], 1 + np.cumsum(np.bincount(c, minlength=n))]).astype(np.int64)
    return cp.SparseMatrixCSC(m, n, colptr, r + 1)


def edge_shape(n):
    """tests/test_gpu_scale_parity.edge_shapes scaled down: a row in every column, one column of n/4 entries, n/40 consecutive columns
    without entries, and rows that are never hit (n .. m - 1)"""
    rng = np.random.default_rng(2024 + n)
    m = n + n // 2
    c = rng.integers(0, n, 5 * n); r = np.clip(c + rng.normal(0, n / 50, c.size).astype(np.int64), 0, n - 1)
    c = np.concatenate([c, np.arange(n), np.full(n // 4, n // 3)]); r = np.concatenate([r, np.full(n, 77), np.arange(n // 4) * 2])
    keep = (c < n // 4) | (c >= n // 4 + n // 40)
    return _from_entries(m, n, c[keep], r[keep])


class Pat:
    """a pattern and, built once each, its transforms"""

    def __init__(self, A, seed):
        self.A, self.seed, self._made = A, seed, {}

    def get(self, how):
        if how not in self._made:
            A, rng = self.A, np.random.default_rng(self.seed)
            make = {"relabel": lambda: mm.relabel_rows(A, rng, return_map=True), "relabel777": lambda: mm.relabel_rows(A, rng, 777, return_map=True),
                    "mirror": lambda: mm.mirror_columns(A), "reverse": lambda: mm.reverse_rows(A), "shift": lambda: mm.shift_rows(A, 1000)}
            self._made[how] = make[how]()
        return self._made[how]


@functools.lru_cache(maxsize=None)
def pat(name, n):
    return Pat({"ss": lambda: suitesparse_shaped(n, 8, 11), "band": lambda: banded(n, 6, 0.5, 12), "edge": lambda: edge_shape(n)}[name](), n)


def grid(n):
    """(pattern, K): every pairing at n = 4 099, one per pattern at n = 70 001"""
    if n == TINY:
        return (("ss", 7),)
    if n >= REDUCED:
        return (("ss", 16), ("band", 7), ("edge", 16))
    return tuple((name, K) for name in ("ss", "band", "edge") for K in (7, 16))


def limit(A, K, kind):
    """the constraint of a case -> None | ("w", width) | ("pins", budget)"""
    n = A.n
    return {None: None, "w15": ("w", math.ceil(1.5 * n / K)), "w11": ("w", math.ceil(1.1 * n / K)), "pins": ("pins", math.ceil(1.3 * A.nnz / K)),
            "cw3": ("w", 3), "cw17": ("w", 17), "cw64": ("w", 64), "cwq": ("w", n // 4)}[kind]


def kw(con):
    """the constraint as pair_slack / greedy_parts / structure_ok take it"""
    return {} if con is None else {"w": con[1]} if con[0] == "w" else {"budget": con[1]}


# ---------------------------------------------------------------- the solver
TOTAL_SLOTS = ("dp_lpass", "dp_open_segments", "dp_task_setup", "dp_tile_carry", "dp_span_fix", "dp_combine", "dp_rpass", "dp_lpass_own",
               "dp_gap_finish", "dp_lpass_gap", "dp_round_a", "dp_leaf")


class Lib:
    """lib(A, K, method, mdl, con, Pi) -> the split vector, on a backend.  On the device at n >= SCALE: no O(n^2) sweep, and with
    engine=... the named engine must have run."""

    def __init__(self, backend):
        self.b = backend
        self.hip = getattr(backend, "name", "") == "hip"
        self.memo = {}

    @contextlib.contextmanager
    def _guard(self, engine):
        b = self.b
        b.set_option("brute_max_n", 0)
        if engine:
            b.set_option("stat_reset", 0)
            b.prof_reset(); b.prof_enable(True)
        try:
            yield
        finally:
            b.prof_enable(False)
            b.set_option("brute_max_n", 200000)
        if engine:
            p = b.prof_get()
            ran = lambda slot: p[slot]["launches"] > 0
            seen = {"Total": any(ran(s) for s in TOTAL_SLOTS) and not ran("chunker") and not ran("dp_brute") and not ran("dp_budget"),
                    "Budget": ran("dp_budget") and b.get_stat("budget_layers") > 0 and not ran("chunker"),
                    "Valley": ran("dp_brute") and not ran("chunker"),
                    "EnvDc": ran("env_dc") and b.get_stat("env_dc_layers") > 0 and not ran("env_sweep"),
                    "EnvValley": ran("env_valley") and b.get_stat("env_valley_layers") > 0 and not ran("env_sweep"),
                    "Lws": ran("chunk_lws"),
                    "CutScan": b.get_stat("cut_scan_layers") > 0,
                    "SymTotal": ran("dp_sym_total") and b.get_stat("sym_total_layers") > 0 and not ran("dp_brute"),
                    "PlaidTotal": ran("dp_plaid_total") and b.get_stat("plaid_total_layers") > 0 and not ran("dp_brute"),
                    "PlaidScan": ran("dp_plaid_total") and b.get_stat("plaid_scan_layers") > 0 and not ran("dp_brute")}[engine]
            assert seen, (engine, {s: v["launches"] for s, v in p.items() if v["launches"]})

    def __call__(self, A, K, method, mdl, con=None, Pi=None, engine=None):
        f = mdl if con is None else cp.ConstrainedCost(mdl, cp.VertexCount() if con[0] == "w" else PINS, con[1])
        guard = self._guard(engine) if self.hip and A.n >= SCALE else contextlib.nullcontext()
        with guard:
            if method in PACK:
                return cp.pack_stripe(A, PACK[method](f), backend=self.b).spl
            return cp.partition_stripe(A, K, METHODS[method](f), Pi, backend=self.b).spl

    def base(self, A, K, case, mdl, con, Pi=None):
        """the case's own call, once (and once with the engine check)"""
        key = (id(A), K, case.id, key_of(mdl), con, id(Pi))
        if key not in self.memo:
            self.memo[key] = (A, Pi, self(A, K, case.method, mdl, con, Pi, engine=case.engine_at(A.n, con)))
        return self.memo[key][2]


@pytest.fixture(scope="module")
def lib(hip):
    return Lib(hip)


# ---------------------------------------------------------------- the cases
class Case(namedtuple("Case", "id method con objective engine at_scale at_small exact at_tiny", defaults=((),))):
    """objective: "sum" | "max"; engine: what must run at n >= SCALE; at_scale / at_small / at_tiny: the models at n >= SCALE, below it and
    at n = TINY (the one-wave routes); exact: the answer is an optimum"""

    def engine_at(self, n, con):
        if self.engine == "Lws" and con is not None and con[1] <= 16:        # (the narrow widths have a kernel of their own)
            return None
        return self.engine

    def models(self, n):
        return self.at_scale if n >= SCALE else self.at_tiny if n == TINY else self.at_small

    def sizes(self):
        """pack_stripe(ConvexTotalChunker) at w = n / 4 walks its stack on one wave, 7 s a call at n = 70 001: it runs at 20 001"""
        big = REDUCED if self.id == "pack_convex-cwq" else SCALE
        return ((TINY,) if self.at_tiny else ()) + (SMALL,) + ((big,) if self.at_scale else ())

    @property
    def splitter(self):
        return self.method in ("total", "bottleneck", "bisect_index")


CASES = []
for _m in ("total", "total_chunker"):
    CASES.append(Case(_m, _m, None, "sum", "Total", MONGE, ALL + (HCUT_M,), True))
    for _c in ("w15", "w11"):
        CASES.append(Case(f"{_m}-{_c}", _m, _c, "sum", "Total", MONGE, MONGE, True, ONE_WAVE_TOTAL))
    CASES.append(Case(f"{_m}-pins", _m, "pins", "sum", "Budget", MONGE, MONGE, True, ONE_WAVE_TOTAL))
CASES.append(Case("bottleneck", "bottleneck", None, "max", "Valley", ALL, ALL, True))
for _c in ("w15", "w11", "pins"):
    CASES.append(Case(f"bottleneck-{_c}", "bottleneck", _c, "max", "Valley", INT, INT, True, ONE_WAVE_BOTTLENECK))
CASES.append(Case("bisect_index", "bisect_index", None, "max", None, BISECTED, BISECTED, True))
CASES.append(Case("bisect_cost", "bisect_cost", None, "max", None, BISECTED, BISECTED, False))
CASES.append(Case("lazy", "lazy", None, "max", None, CONN, CONN, False))
for _c in ("cw3", "cw17", "cw64", "cwq"):
    CASES.append(Case(f"pack_dynamic-{_c}", "pack_dynamic", _c, "sum", "Lws", MONGE, MONGE, True, ONE_WAVE_TOTAL))
    # (ConvexTotalChunker presumes a cost its candidate stack is valid for: with HCUT, self > cut, the reference's own answer is neither
    #  pair-optimal nor mirror-invariant -- oracle, banded(1200, 6, 0.5, 5), w = 17 -- so that pair stays out)
    CASES.append(Case(f"pack_convex-{_c}", "pack_convex", _c, "sum", None, (CONN_I, WORK), MONGE, True, (CONN_D,)))
BY_ID = {c.id: c for c in CASES}
DP = [c for c in CASES if c.method in ("total", "total_chunker", "bottleneck") or c.method in PACK]
BISECT = [c for c in CASES if c.method in ("bisect_index", "bisect_cost", "lazy")]
ids = lambda cases: [c.id for c in cases]


def per_size(cases):
    """one test per case and size it runs at; the id names the size that runs"""
    pairs = [(c, n) for c in cases for n in c.sizes()]
    return pytest.mark.parametrize("case,n", pairs, ids=[f"{c.id}-{n}" for c, n in pairs])


def runs(case, n):
    """(Pat, K, model, constraint) of a case at a size"""
    for name, K in grid(n):
        P = pat(name, n)
        for mdl in case.models(n):
            yield P, K, mdl, limit(P.A, K, case.con)


def nondegenerate(case, spl, what):
    """a constrained or bottleneck answer that feeds a value check decides something (the unconstrained total optimum is the closed
    form [1, n + 1, ...] and takes part in the identities only)"""
    if case.con is not None or case.objective == "max":
        assert len(set(np.asarray(spl).tolist())) > 3, (case.id, what, spl)


def value(case, A, mdl, spl, Pi=None):
    return (mm.total if case.objective == "sum" else mm.bottleneck)(A, mdl, spl, Pi)


# ---------------------------------------------------------------- the relations (also run on the oracle by tests/test_meta_model.py)
def check_structure(lib, case, P, K, mdl, con):
    spl = lib.base(P.A, K, case, mdl, con)
    assert mm.structure_ok(P.A, spl, **kw(con)), (case.id, K, key_of(mdl), con, spl)
    if case.method not in PACK:
        assert len(spl) == K + 1


def check_relabel(lib, case, P, K, mdl, con):
    spl = lib.base(P.A, K, case, mdl, con)
    for how in ("relabel", "relabel777"):
        got = lib(P.get(how)[0], K, case.method, mdl, con)
        assert np.array_equal(got, spl), (case.id, how, K, key_of(mdl), con, got, spl)


def check_mirror(lib, case, P, K, mdl, con):
    spl = lib.base(P.A, K, case, mdl, con)
    nondegenerate(case, spl, "mirror")
    B = P.get("mirror")
    got = lib.base(B, K, case, mdl, con)
    assert value(case, B, mdl, got) == value(case, P.A, mdl, spl), (case.id, K, key_of(mdl), con, got, spl)


def check_scaling(lib, case, P, K, mdl, con, factors=(3, 1 << 20)):
    spl = lib.base(P.A, K, case, mdl, con)
    for c in factors:
        got = lib(P.A, K, case.method, mm.scaled(mdl, c), con)
        assert np.array_equal(got, spl), (case.id, c, K, key_of(mdl), con, got, spl)


def check_shift(lib, case, P, K, mdl, con):
    spl = lib.base(P.A, K, case, mdl, con)
    got = lib(P.A, K, case.method, mm.shifted(mdl, 12345), con)
    assert np.array_equal(got, spl), (case.id, K, key_of(mdl), con, got, spl)


def check_pair(lib, case, P, K, mdl, con):
    spl = lib.base(P.A, K, case, mdl, con)
    nondegenerate(case, spl, "pair")
    slack = mm.pair_slack(P.A, mdl, spl, **kw(con))
    assert all(s == 0 for s in slack), (case.id, K, key_of(mdl), con, spl, slack)


def check_certificate(lib, case, P, K, mdl, con):
    spl = lib.base(P.A, K, case, mdl, con)
    nondegenerate(case, spl, "certificate")
    c = mm.bottleneck(P.A, mdl, spl)
    assert mm.certified(P.A, mdl, K, c, step=step_of(mdl), **kw(con)), (case.id, K, key_of(mdl), con, spl, c)


def check_within_eps(lib, case, P, K, mdl, con):
    spl = lib.base(P.A, K, case, mdl, con)
    nondegenerate(case, spl, "within eps")
    assert mm.structure_ok(P.A, spl)
    opt = mm.bottleneck_optimum(P.A, mdl, K, step=step_of(mdl))
    assert opt <= mm.bottleneck(P.A, mdl, spl) <= (1 + EPS) * opt, (case.id, K, key_of(mdl), spl, opt)


def check_relaxation(lib, method, P, K, mdl, bound=None):
    """w >= n and budget >= nnz give the unconstrained split; the optimum does not rise as w or the budget grows, nor (alpha = 0) from
    K to K + 1.  A model outside the constrained cases of its method (the one-wave routes) takes part from K to K + 1 only."""
    A = P.A
    case = BY_ID[method]
    free = lib.base(A, K, case, mdl, None)
    v = lambda spl: value(case, A, mdl, spl)
    if bound is None:                                              # (the reference serves every pair at every size)
        bound = mdl in BY_ID[method + "-w15"].models(A.n)
    if bound:
        for con in (("w", A.n), ("w", A.n + 3), ("pins", A.nnz), ("pins", A.nnz + 5)):
            got = lib(A, K, method, mdl, con)
            assert np.array_equal(got, free), (method, K, key_of(mdl), con, got, free)
        at = {kind: v(lib.base(A, K, BY_ID[f"{method}-{kind}"], mdl, limit(A, K, kind))) for kind in ("w15", "w11", "pins")}
        assert v(free) <= at["w15"] <= at["w11"] and v(free) <= at["pins"], (method, K, key_of(mdl), v(free), at)
    if mdl.alpha == 0:
        for kind in (None, "w15", "pins") if bound else (None,):
            con = limit(A, K, kind)                                # (the limits of K, kept for K + 1)
            more = lib(A, K + 1, method, mdl, con)
            assert mm.structure_ok(A, more, **kw(con))
            assert v(more) <= v(lib.base(A, K, BY_ID[method if kind is None else f"{method}-{kind}"], mdl, con)), (method, kind, K, key_of(mdl))


# ---------------------------------------------------------------- the tests: one per relation, case and size
SIZES = pytest.mark.parametrize("n", [SMALL, SCALE])


@per_size(CASES)
def test_structure(lib, case, n):
    for args in runs(case, n):
        check_structure(lib, case, *args)


@per_size(CASES)
def test_row_relabelling(lib, case, n):
    for args in runs(case, n):
        check_relabel(lib, case, *args)


@per_size([c for c in CASES if c.exact])
def test_mirror(lib, case, n):
    for args in runs(case, n):
        check_mirror(lib, case, *args)


@per_size(DP)
def test_scaling(lib, case, n):
    for args in runs(case, n):
        check_scaling(lib, case, *args)


def check_scaling_bisect(lib, case, P, K, mdl, con):
    """BisectIndex returns the chain of its optimal cost, whatever the scale.  The cost bisections start from bounds that hold a floor
    (alpha + floor(s / K), Costs.jl:17-19), which a factor moves by a fraction of a unit: the reference's own loop then probes between
    other costs (banded(1200, 6, 0.5, 5), K = 16, AffineWorkModel(0, 10, 1) times 2^20), so what holds for them is their property, on
    the scaled model too"""
    got = lib(P.A, K, case.method, mm.scaled(mdl, 1 << 20), con)
    if case.exact:
        spl = lib.base(P.A, K, case, mdl, con)
        assert np.array_equal(got, spl), (case.id, K, key_of(mdl), got, spl)
    else:
        opt = mm.bottleneck_optimum(P.A, mdl, K, step=step_of(mdl))
        assert mm.structure_ok(P.A, got) and opt <= mm.bottleneck(P.A, mdl, got) <= (1 + EPS) * opt, (case.id, K, key_of(mdl), got, opt)


@per_size(BISECT)
def test_scaling_by_a_power_of_two_on_the_bisections(lib, case, n):
    for args in runs(case, n):
        check_scaling_bisect(lib, case, *args)


@per_size([c for c in CASES if c.splitter])
def test_shift(lib, case, n):
    for args in runs(case, n):
        check_shift(lib, case, *args)


@SIZES
@pytest.mark.parametrize("method", ["total", "total_chunker", "bottleneck"])
def test_relaxation(lib, method, n):
    for name, K in grid(n):
        for mdl in BY_ID[method].models(n):
            check_relaxation(lib, method, pat(name, n), K, mdl)
    if n == SMALL:                                                 # the one-wave pairs, at their size
        for name, K in grid(TINY):
            for mdl in BY_ID[method + "-w15"].at_tiny:
                check_relaxation(lib, method, pat(name, TINY), K, mdl)


@per_size([c for c in DP if c.objective == "sum"])
def test_pairwise_optimality(lib, case, n):
    for args in runs(case, n):
        check_pair(lib, case, *args)


CERTIFIED = [c for c in CASES if c.objective == "max" and c.exact]


@per_size(CERTIFIED)
def test_bottleneck_certificate(lib, case, n):
    for args in runs(case, n):
        check_certificate(lib, case, *args)


APPROX = [c for c in CASES if not c.exact]


@per_size(APPROX)
def test_bisections_within_eps_of_the_optimum(lib, case, n):
    """the reference's own property (test_Partitioners.jl:112)"""
    for args in runs(case, n):
        check_within_eps(lib, case, *args)


@SIZES
def test_lazy_flip_within_eps_of_the_optimum(lib, n):
    """a decreasing cost c0 - g(j, j') with g growing: its least bottleneck is c0 minus the greatest achievable least g, which the greedy
    cover finds (the flip relation of tests/test_gpu_lazy_flip.py, with the host greedy in the place of FlipBisectIndex)"""
    for name, K in grid(n):
        P = pat(name, n)
        A = P.A
        c0 = 1 + A.nnz + 3 * A.n + 3 * A.m
        dec, g = cp.AffineConnectivityModel(c0, -3, -1, -3), cp.AffineConnectivityModel(0, 3, 1, 3)
        # (the method takes its upper bound from the per-part alphas: the decreasing model goes in that form, as in the reference's tests)
        asked = lambda c: cp.AffineConnectivityModel(0, -3 * c, -c, -3 * c, alpha_k=[c0 * c] * K)
        spl = lib(A, K, "lazy_flip", asked(1))
        assert mm.structure_ok(A, spl) and len(set(spl.tolist())) > 3
        opt = c0 - mm.maxmin_optimum(A, g, K)
        assert opt <= mm.bottleneck(A, dec, spl) <= (1 + EPS) * opt, (name, K, spl, opt)
        for how in ("relabel", "relabel777"):
            assert np.array_equal(lib(P.get(how)[0], K, "lazy_flip", asked(1)), spl), (name, K, how)
        got = lib(A, K, "lazy_flip", asked(1 << 20))
        assert mm.structure_ok(A, got) and opt <= mm.bottleneck(A, dec, got) <= (1 + EPS) * opt, (name, K, got, opt)


# ---------------------------------------------------------------- the envelope cost
ENV_CASES = [Case("env_total", "total", None, "sum", "EnvDc", (ENV,), (ENV,), True), Case("env_bottleneck", "bottleneck", None, "max", "EnvValley", (ENV,), (ENV,), True)]


def check_envelope(lib, case, P, K):
    A = P.A
    spl = lib.base(A, K, case, ENV, None)
    assert mm.structure_ok(A, spl) and len(spl) == K + 1
    if case.objective == "max":                                    # (the total optimum is one part, like the unconstrained total)
        assert len(set(spl.tolist())) > 3, (case.id, spl)
    for how in ("reverse", "shift"):
        got = lib(P.get(how), K, case.method, ENV)
        assert np.array_equal(got, spl), (case.id, how, K, got, spl)
    B = P.get("mirror")
    assert value(case, B, ENV, lib.base(B, K, case, ENV, None)) == value(case, A, ENV, spl), (case.id, K)
    for mdl in (mm.scaled(ENV, 3), mm.scaled(ENV, 1 << 20), mm.shifted(ENV, 12345)):
        got = lib(A, K, case.method, mdl)
        assert np.array_equal(got, spl), (case.id, key_of(mdl), K, got, spl)
    assert value(case, A, ENV, lib(A, K + 1, case.method, ENV)) <= value(case, A, ENV, spl)
    if case.objective == "sum":
        # a negative span term pays for the rows that neighbouring parts share: a total optimum with many parts in use
        for mdl in (ENV, ENV_SPREAD):
            got = spl if mdl is ENV else lib(A, K, case.method, mdl)
            slack = mm.pair_slack(A, mdl, got)
            assert all(s == 0 for s in slack), (case.id, key_of(mdl), K, got, slack)
            B = P.get("mirror")
            assert mm.total(B, mdl, lib(B, K, case.method, mdl)) == mm.total(A, mdl, got), (case.id, key_of(mdl), K)
            if mdl is ENV_SPREAD:
                assert len(set(got.tolist())) > 3, (case.id, got)
    else:
        assert mm.certified(A, ENV, K, mm.bottleneck(A, ENV, spl)), (case.id, K, spl)


@per_size(ENV_CASES)
def test_envelope(lib, case, n):
    for name, K in grid(n):
        check_envelope(lib, case, pat(name, n), K)


# ---------------------------------------------------------------- the plaid costs under a MapPartition of the rows
PLAID_CASES = [Case("plaid_cut", "total", None, "sum", "CutScan", (PCUT,), (PCUT,), True), Case("plaid_connectivity", "total", None, "sum", None, (), (PRIM,), True)]


def row_map(A, K, seed):
    """rows in K bands along the diagonal, one in ten thrown anywhere"""
    rng = np.random.default_rng(seed)
    asg = 1 + (np.arange(A.m, dtype=np.int64) * K) // A.m
    stray = rng.random(A.m) < 0.1
    asg[stray] = rng.integers(1, K + 1, int(stray.sum()))
    return cp.MapPartition(K, asg)


def check_plaid(lib, case, P, K, mdl):
    A = P.A
    Pi = P._made.setdefault(("rows", K), row_map(A, K, 5 + K))
    spl = lib.base(A, K, case, mdl, None, Pi)
    assert mm.structure_ok(A, spl) and len(spl) == K + 1
    if mdl is PCUT:                                                # (the connectivity optimum is one part, like the unconstrained total)
        assert len(set(spl.tolist())) > 3, (case.id, spl)
    for how in ("relabel", "relabel777"):
        B, sigma = P.get(how)
        asg = np.ones(B.m, dtype=np.int64)
        asg[sigma] = Pi.asg                                        # asg'[sigma] = asg; the empty extras go anywhere
        got = lib(B, K, case.method, mdl, None, cp.MapPartition(K, asg))
        assert np.array_equal(got, spl), (case.id, how, K, got, spl)
    for other in (mm.scaled(mdl, 3), mm.scaled(mdl, 1 << 20), mm.shifted(mdl, 12345)):
        got = lib(A, K, case.method, other, None, Pi)
        assert np.array_equal(got, spl), (case.id, key_of(other), K, got, spl)
    slack = mm.pair_slack(A, mdl, spl, Pi=Pi)
    assert all(s == 0 for s in slack), (case.id, K, spl, slack)


@pytest.mark.parametrize("case,n", [(PLAID_CASES[0], SMALL), (PLAID_CASES[0], SCALE), (PLAID_CASES[1], SMALL)],
                         ids=["plaid_cut-4099", "plaid_cut-70001", "plaid_connectivity-4099"])
def test_plaid(lib, case, n):
    for name, K in grid(n):
        for mdl in case.models(n):
            check_plaid(lib, case, pat(name, n), K, mdl)


# ---------------------------------------------------------------- the symmetric family and the plaid connectivity pair, total objective
SYM_CASE = Case("sym_total", "total", None, "sum", "SymTotal", SYM, SYM, True)
PRIMARY_CASE = Case("plaid_connectivity", "total", None, "sum", "PlaidTotal", (PRIM, PRIM_BAND), (PRIM, PRIM_BAND), True)
SECONDARY_CASE = Case("plaid_secondary", "total", None, "sum", "PlaidScan", (SECOND,), (SECOND,), True)


def check_total_relations(lib, case, A, K, mdl, Pi, mirrored, many_parts):
    """structure; the value on the mirrored problem; the split vector under a factor of 3 and 2^20 and under a shift; pair_slack == 0;
    alpha = 0: K + 1 parts cost no more (where part K + 1 may stay empty at no cost).  mirrored: (pattern, partition) of the mirror"""
    spl = lib.base(A, K, case, mdl, None, Pi)
    assert mm.structure_ok(A, spl) and len(spl) == K + 1, (case.id, K, spl)
    if many_parts:
        assert len(set(spl.tolist())) > 3, (case.id, key_of(mdl), K, spl)
    B, Pj = mirrored
    got = lib.base(B, K, case, mdl, None, Pj)
    assert mm.total(B, mdl, got, Pj) == mm.total(A, mdl, spl, Pi), (case.id, key_of(mdl), K, got, spl)
    for other in (mm.scaled(mdl, 3), mm.scaled(mdl, 1 << 20), mm.shifted(mdl, 12345)):
        got = lib(A, K, case.method, other, None, Pi)
        assert np.array_equal(got, spl), (case.id, key_of(other), K, got, spl)
    slack = mm.pair_slack(A, mdl, spl, Pi=Pi)
    assert all(x == 0 for x in slack), (case.id, key_of(mdl), K, spl, slack)
    if mdl.alpha == 0 and case is not SECONDARY_CASE:               # (a secondary part costs its rows and pins even without a column)
        more = lib(A, K + 1, case.method, mdl, None, Pi)
        assert mm.structure_ok(A, more) and mm.total(A, mdl, more, Pi) <= mm.total(A, mdl, spl, Pi), (case.id, key_of(mdl), K, more, spl)


def check_sym(lib, case, P, K, mdl):
    mirrored = P._made.setdefault("mirror_both", mm.mirror_both(P.A))
    check_total_relations(lib, case, P.A, K, mdl, None, (mirrored, None), False)


def check_primary(lib, case, P, K, mdl, name):
    """banded owners; on the mirrored columns the parts run the other way, so part k's rows become part K + 1 - k's"""
    A = P.A
    Pi = P._made.setdefault(("rows", K), row_map(A, K, 5 + K))
    Pj = P._made.setdefault(("rows mirrored", K), cp.MapPartition(K, K + 1 - np.asarray(Pi.asg, dtype=np.int64)))
    # where every row lies within a few columns of the diagonal a part that follows its rows pays for the strayed rows only
    check_total_relations(lib, case, A, K, mdl, Pi, (P.get("mirror"), Pj), mdl is PRIM_BAND and name == "band")


def check_secondary(lib, case, P, K, mdl, name):
    """an even SplitPartition of the rows; the mirror turns rows and columns round, and with them the order of the parts"""
    A = P.A
    cuts = np.linspace(1, A.m + 1, K + 1).astype(np.int64)
    Phi = P._made.setdefault(("split", K), cp.SplitPartition(K, cuts))
    B = P._made.setdefault("mirror reversed", mm.mirror_columns(mm.reverse_rows(A)))
    Phj = P._made.setdefault(("split mirrored", K), cp.SplitPartition(K, (A.m + 2 - cuts)[::-1].copy()))
    check_total_relations(lib, case, A, K, mdl, Phi, (B, Phj), name in ("ss", "band"))


@pytest.mark.parametrize("n", [SMALL, SCALE])
@pytest.mark.parametrize("mdl", SYM, ids=["sym_conn", "mono_sym", "edge_cut"])
def test_symmetric_total(lib, mdl, n):
    for name, K in grid(n):
        if name != "edge":                                         # (the edge shape is not square)
            check_sym(lib, SYM_CASE, pat(name, n), K, mdl)


@pytest.mark.parametrize("n", [SMALL, SCALE])
def test_plaid_connectivity_total(lib, n):
    for name, K in grid(n):
        for mdl in PRIMARY_CASE.models(n):
            check_primary(lib, PRIMARY_CASE, pat(name, n), K, mdl, name)


@pytest.mark.parametrize("n", [SMALL, SCALE])
def test_plaid_secondary_total(lib, n):
    for name, K in grid(n):
        check_secondary(lib, SECONDARY_CASE, pat(name, n), K, SECOND, name)
