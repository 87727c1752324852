"""Which engine runs a layer of the K-layer dynamic programme (csrc/dp_driver.hip), for every family of (model, objective, loop
order, weight, options) the driver tells apart.  Every path is exact, so a wrong route still gives the right answer, only orders of
magnitude slower: the route is read from what the library already reports -- the status, the profile slots and the stats.

A path name is what path_of() makes of those observables:
  Total / Windowed        a slot of the O(n log^2 n) scheme ticks (Windowed: under a ConstrainedCost)
  Valley / Sweep          dp_brute ticks; the valley search still runs with brute_max_n = 0, the O(n^2) sweep is refused ("n too large")
  SymValley               ... and bn_sym_layers counts
  EnvValley / EnvDc / EnvSweep   the envelope slots (and their stats)
  Budget                  dp_budget ticks and budget_layers counts
  OneWave                 chunker ticks: the one-wave literal kernel of seq.hip
  CP_EUNSUPPORTED / CP_EINVAL    refused
and every case that returns an answer returns the oracle's."""
import contextlib
import functools

import numpy as np
import pytest

import envelope_model as em
import sym_model as sm
from test_gpu_budget_total import profiled
from test_gpu_envelope import pattern as env_pattern
from test_gpu_symmetric import MODELS_I as SYM_I, pattern as sym_pattern, tables as sym_tables
from util import cp, suitesparse_shaped

pytestmark = pytest.mark.gpu

M = cp.models
K = 4
SUM, MAX = M.CP_COMBINE_SUM, M.CP_COMBINE_MAX
TOTAL_SLOTS = ("dp_lpass", "dp_open_segments", "dp_task_setup", "dp_tile_carry", "dp_span_fix", "dp_combine", "dp_rpass", "dp_lpass_own",
               "dp_gap_finish", "dp_lpass_gap", "dp_round_a", "dp_leaf")
SLOTS = {"dp_brute": "brute", "chunker": "OneWave", "dp_budget": "Budget", "env_valley": "EnvValley", "env_sweep": "EnvSweep", "env_dc": "EnvDc"}
STATS = {"budget_layers": "Budget", "env_dc_layers": "EnvDc", "env_valley_layers": "EnvValley", "bn_sym_layers": "SymValley"}
METHODS = {(SUM, "splitter"): cp.DynamicTotalSplitter, (SUM, "chunker"): cp.DynamicTotalChunker,
           (MAX, "splitter"): cp.DynamicBottleneckSplitter, (MAX, "chunker"): cp.DynamicBottleneckChunker}
ORDER = {"splitter": M.CP_ORDER_SPLITTER, "chunker": M.CP_ORDER_CHUNKER}

CONN = cp.AffineConnectivityModel(0, 3, 1, 3)
CONN_F = cp.AffineConnectivityModel(0.0, 3.0, 1.0, 3.0)
CONN_FRAC = cp.AffineConnectivityModel(0.5, 0.25, 0.0, 1.5)
CONN_AK = cp.AffineConnectivityModel(0, 3, 1, 3, alpha_k=[5, 1, 9, 2, 7, 3, 8, 4])
WORK = cp.AffineWorkModel(-3, 1, 0)
HCUT = cp.AffineHyperedgeCutModel(0, 1, 1, 1, 3)
COLBLOCK = cp.ColumnBlockComponentCostModel(3, lambda x: 1 + x)
ENV = cp.AffineEnvelopeModel(0, 10, 1, 100)
ENV_NEG = cp.AffineEnvelopeModel(0, 1, -1, 2)
MONO = SYM_I[1]
PINS = cp.AffineWorkModel(0, 0, 1)


@functools.lru_cache(maxsize=None)
def mat(name="stripe"):
    """one matrix per family, built once (and one device handle each)"""
    if name == "sym":
        return sym_pattern(257, "partial")
    if name == "env":
        return env_pattern(40, 300, 6, dens=0.1)
    return suitesparse_shaped(300, 6, 9)


@contextlib.contextmanager
def options(hip, opts):
    """opts: ((name, value, the default to restore), ...)"""
    try:
        for name, value, _ in opts:
            hip.set_option(name, value)
        yield
    finally:
        for name, _, default in opts:
            hip.set_option(name, default)


def observe(hip, call):
    """-> (the status name of a refusal | None, its text | the answer, {engines whose slots ticked}, {engines whose stats counted})"""
    hip.set_option("stat_reset", 0)
    with profiled(hip):
        try:
            out = call()
        except NotImplementedError as e:
            return "CP_EUNSUPPORTED", str(e), set(), set()
        except AssertionError as e:
            return "CP_EINVAL", str(e), set(), set()
    p = hip.prof_get()
    ticked = {name for slot, name in SLOTS.items() if p[slot]["launches"] > 0}
    if any(p[slot]["launches"] > 0 for slot in TOTAL_SLOTS):
        ticked.add("Total")
    return None, out, ticked, {name for stat, name in STATS.items() if hip.get_stat(stat) > 0}


def path_of(hip, call, constrained=False):
    """-> (path name, answer | refusal text)"""
    refused, out, ticked, counted = observe(hip, call)
    if refused:
        return refused, out
    assert len(ticked) <= 1, ticked                                      # one engine per run
    assert counted - {"SymValley"} == ticked & {"Budget", "EnvDc", "EnvValley"}, (ticked, counted)
    name = next(iter(ticked), "None")
    if "SymValley" in counted:
        assert name == "brute"
        name = "SymValley"
    # the valley search and the O(n^2) sweep both time under dp_brute: only the sweeps need n <= brute_max_n
    with options(hip, (("brute_max_n", 0, 200000),)):
        again = observe(hip, call)
    if again[0]:
        assert again[0] == "CP_EUNSUPPORTED" and "n too large" in again[1] and name in ("brute", "EnvSweep"), (name, again)
        name = "Sweep" if name == "brute" else name
    else:
        assert again[2:] == (ticked, counted), (name, again)
        name = "Valley" if name == "brute" else name
    if constrained:
        name = {"Total": "Windowed", "Valley": "Valley with limits"}.get(name, name)
    return name, out


def direct(hip, A, combine, order, mdl, wgt=None, wmax=0):
    """cp_partition_dynamic itself, past the refusals api.py raises before it marshals"""
    spl = np.zeros(K + 1, dtype=np.int64)
    rc = hip.partition_dynamic(A, K, combine, ORDER[order], mdl.marshal(), None, None if wgt is None else wgt.marshal(), int(wmax), float(wmax), spl)
    return raised(hip, rc, spl)


def raised(hip, rc, out):
    if rc == M.CP_EUNSUPPORTED:
        raise NotImplementedError(hip.last_error())
    if rc == M.CP_EINVAL:
        raise AssertionError(hip.last_error())
    assert rc in (M.CP_OK, M.CP_INFEASIBLE), (rc, hip.last_error())
    return out


def tables_entry(hip, A, combine, f):
    """cp_dynamic_tables_constrained_combine -> (rc, j'_lo, j'_hi, ptr, cst)"""
    mdl, wgt, wmax = M.split_constraint(f)
    out = hip.dynamic_tables_constrained(A, K, mdl.marshal(w_table=A.n + 1), wmax, combine=combine, wm=wgt.marshal())      # (w_table: a column-block closure)
    return raised(hip, out[0], out)


# ---------------------------------------------------------------- unconstrained
# (id, matrix, model, objective, loop order, options, path)
FORCE = (("force_brute", 1, 0),)
FREE = []
for _id, _mdl in (("conn_i64", CONN), ("conn_f64", CONN_F), ("work", WORK), ("hcut", HCUT), ("conn_alpha_k", CONN_AK)):
    # (the chunker loop order passes no part index: the reference has no such call for a per-part alpha)
    for _order in ("splitter",) if _mdl.alpha_k is not None else ("splitter", "chunker"):
        FREE.append((f"{_id}-sum-{_order}", "stripe", _mdl, SUM, _order, (), "Total"))
        FREE.append((f"{_id}-sum-{_order}-force_brute", "stripe", _mdl, SUM, _order, FORCE, "Sweep"))
for _id, _mdl in (("conn_frac", CONN_FRAC), ("conn_neg_net", cp.AffineConnectivityModel(0, 3, 1, -3)), ("hcut_self_gt_cut", cp.AffineHyperedgeCutModel(0, 1, 1, 3, 1)),
                  ("conn_2_58", cp.AffineConnectivityModel(0, 1 << 58, 1, 3)), ("colblock", COLBLOCK), ("powerwork", cp.ConcaveWorkModel(0.5, 1, 1))):
    FREE.append((f"{_id}-sum", "stripe", _mdl, SUM, "splitter", (), "Sweep"))
for _id, _mdl in (("conn_i64", CONN), ("conn_frac", CONN_FRAC), ("hcut_self_ge_cut", cp.AffineHyperedgeCutModel(0, 1, 1, 3, 1))):
    FREE.append((f"{_id}-max", "stripe", _mdl, MAX, "splitter", (), "Valley"))
for _id, _mdl in (("hcut_frac", cp.AffineHyperedgeCutModel(0.0, 0.0, 0.0, 0.7, 0.1)), ("conn_neg_vertex", cp.AffineConnectivityModel(0, -1, 1, 3))):
    FREE.append((f"{_id}-max", "stripe", _mdl, MAX, "splitter", (), "Sweep"))
FREE.append(("mono_sym-max", "sym", MONO, MAX, "splitter", (), "SymValley"))
FREE.append(("mono_sym-sum", "sym", MONO, SUM, "splitter", (), "Sweep"))
for _id, _mdl in (("sym_conn", SYM_I[0]), ("sym_edge_cut", SYM_I[2])):
    for _g in (SUM, MAX):
        FREE.append((f"{_id}-{'max' if _g else 'sum'}", "sym", _mdl, _g, "splitter", (), "Sweep"))
FREE.append(("env-max", "env", ENV, MAX, "splitter", (), "EnvValley"))
FREE.append(("env-sum", "env", ENV, SUM, "splitter", (), "EnvDc"))
FREE.append(("env-sum-below_min_n", "env", ENV, SUM, "splitter", (("env_dc_min_n", 301, 256),), "EnvSweep"))
FREE.append(("env-sum-force_brute", "env", ENV, SUM, "splitter", FORCE, "EnvSweep"))
FREE.append(("env_neg-max", "env", ENV_NEG, MAX, "splitter", (), "EnvSweep"))
FREE.append(("env-sum-chunker", "env", ENV, SUM, "chunker", (), "CP_EUNSUPPORTED"))
FREE.append(("env-max-chunker", "env", ENV, MAX, "chunker", (), "CP_EUNSUPPORTED"))


@functools.lru_cache(maxsize=None)
def free_oracle(orc, name, mdl, g, order):
    A = mat(name)
    if name == "sym":
        return sm.dp_partition(sym_tables(257, "partial"), mdl, K, "max" if g else "sum", order)[0]
    if name == "env":
        return em.dp_literal(em.Env(A, mdl), K, "max" if g else "sum")[0]
    return cp.partition_stripe(A, K, METHODS[(g, order)](mdl), backend=orc).spl


@pytest.mark.parametrize("case", FREE, ids=[c[0] for c in FREE])
def test_unconstrained_routing(hip, orc, case):
    _, name, mdl, g, order, opts, want = case
    A = mat(name)
    assert mat("env").n == 300 and mat("env").n >= 256                   # (env_dc_min_n: its default and n + 1 lie on either side)
    if want.startswith("CP_"):                                           # (the library's own refusal: api.py raises one of its own first)
        call = lambda: direct(hip, A, g, order, mdl)
    else:
        call = lambda: cp.partition_stripe(A, K, METHODS[(g, order)](mdl), backend=hip).spl
    with options(hip, opts):
        got, out = path_of(hip, call)
    assert got == want, (case[0], got, out)
    if not want.startswith("CP_"):
        assert np.array_equal(out, free_oracle(orc, name, mdl, g, order)), case[0]


# ---------------------------------------------------------------- constrained
def budgets():
    A = mat()
    pins, width = int(1.3 * A.nnz / K), A.n // 3
    return pins, width


def widths():
    _, w = budgets()
    return (("vertexcount", cp.VertexCount(), w), ("work_0_1_0", cp.AffineWorkModel(0, 1, 0), w), ("work_2_3_0", cp.AffineWorkModel(2, 3, 0), 2 + 3 * w))


def pin_weights():
    b, w = budgets()
    return (("pins", PINS, b), ("work_2_3_1", cp.AffineWorkModel(2, 3, 1), 2 + 3 * w + b), ("work_frac", cp.AffineWorkModel(0.5, 0.0, 0.25), 0.5 + 0.25 * b))


# (id, model, weight, w_max, objective, options, path)
BOUND = []
for _wid, _wgt, _wmax in widths():
    BOUND.append((f"conn-{_wid}-sum", CONN, _wgt, _wmax, SUM, (), "Windowed"))
    BOUND.append((f"conn-{_wid}-max", CONN, _wgt, _wmax, MAX, (), "Valley with limits"))
    BOUND.append((f"conn-{_wid}-max-bn_wave_1", CONN, _wgt, _wmax, MAX, (("bn_wave", 1, 2),), "OneWave"))
for _id, _mdl in (("conn_i64", CONN), ("conn_f64", CONN_F), ("hcut", HCUT), ("work", WORK)):
    for _wid, _wgt, _wmax in pin_weights():
        BOUND.append((f"{_id}-{_wid}-sum", _mdl, _wgt, _wmax, SUM, (), "Budget"))
        BOUND.append((f"{_id}-{_wid}-sum-budget_total_0", _mdl, _wgt, _wmax, SUM, (("budget_total", 0, 1),), "OneWave"))
        BOUND.append((f"{_id}-{_wid}-sum-force_brute", _mdl, _wgt, _wmax, SUM, FORCE, "OneWave"))
BOUND.append(("conn_i64-pins-max", CONN, PINS, budgets()[0], MAX, (), "Valley with limits"))
BOUND.append(("conn_f64-pins-max", CONN_F, PINS, budgets()[0], MAX, (), "OneWave"))
BOUND.append(("colblock-pins-sum", COLBLOCK, PINS, budgets()[0], SUM, (), "OneWave"))
BOUND.append(("conn_frac-pins-sum", CONN_FRAC, PINS, budgets()[0], SUM, (), "OneWave"))
for _g in (SUM, MAX):
    BOUND.append((f"conn-pins_alpha_k-{'max' if _g else 'sum'}", CONN, cp.AffineWorkModel(0, 0, 1, alpha_k=[1, 0, 2, 0]), budgets()[0] + 2, _g, (), "CP_EINVAL"))


@pytest.mark.parametrize("case", BOUND, ids=[c[0] for c in BOUND])
def test_constrained_routing(hip, orc, case):
    """the partition entry, both loop orders, and the tables entry: the same path, or -- where the partition entry falls back to the
    one-wave kernel -- the tables entry's refusal"""
    _, mdl, wgt, wmax, g, opts, want = case
    A = mat()
    f = cp.ConstrainedCost(mdl, wgt, wmax)
    with options(hip, opts):
        for order in ("splitter", "chunker"):
            got, out = path_of(hip, lambda: cp.partition_stripe(A, K, METHODS[(g, order)](f), backend=hip), constrained=True)
            assert got == want, (case[0], order, got, out)
            if want == "CP_EINVAL":
                assert "weight must be VertexCount or an AffineWorkModel" in out
            else:
                part = cp.partition_stripe(A, K, METHODS[(g, order)](f), backend=orc)
                assert out == part and len(set(part.spl.tolist())) > 2, (case[0], order)      # (a budget that decides something)
        got, out = path_of(hip, lambda: tables_entry(hip, A, g, f), constrained=True)
    if want == "OneWave":
        assert got == "CP_EUNSUPPORTED" and "outside the windowed scalable path" in out, (case[0], got, out)
        return
    assert got == want, (case[0], got, out)
    if want != "CP_EINVAL":
        rc2, lo2, hi2, p2, c2 = orc.dynamic_tables_constrained(A, K, g, mdl.marshal(), None, wgt.marshal(), int(wmax), float(wmax))
        rc1, lo1, hi1, p1, c1 = out
        assert rc1 == rc2 == 0
        assert np.array_equal(lo1, lo2) and np.array_equal(hi1, hi2) and np.array_equal(p1, p2) and np.array_equal(c1, c2), case[0]


def test_constrained_refusals(hip):
    """no constrained form: a symmetric, envelope or plaid cost under any weight, and any cost under an envelope weight"""
    pins, width = budgets()
    plaid = (cp.AffinePrimaryConnectivityModel(0, 1, 1, 1, 3), cp.AffineSecondaryConnectivityModel(0, 1, 1, 1, 3), cp.AffinePrimaryEdgeCutModel(0, 1, 1, 3),
             cp.AffineSecondaryEdgeCutModel(0, 1, 1, 3))
    cases = [("sym", mdl, wgt, wmax) for mdl in SYM_I for wgt, wmax in ((cp.VertexCount(), 80), (PINS, 600))]
    cases += [("env", ENV, wgt, wmax) for wgt, wmax in ((cp.VertexCount(), width), (PINS, pins))]
    cases += [("stripe", mdl, wgt, wmax) for mdl in plaid for wgt, wmax in ((cp.VertexCount(), width), (PINS, pins))]
    cases += [(name, mdl, ENV, 10 ** 6) for name, mdl in (("stripe", CONN), ("stripe", WORK), ("env", ENV), ("sym", MONO))]
    for name, mdl, wgt, wmax in cases:
        A = mat(name)
        for g in (SUM, MAX):
            for order in ("splitter", "chunker"):
                got, out = path_of(hip, lambda: direct(hip, A, g, order, mdl, wgt, wmax), constrained=True)
                assert got == "CP_EUNSUPPORTED", (type(mdl).__name__, type(wgt).__name__, g, order, got, out)
            got, out = path_of(hip, lambda: tables_entry(hip, A, g, cp.ConstrainedCost(mdl, wgt, wmax)), constrained=True)
            assert got == "CP_EUNSUPPORTED", (type(mdl).__name__, type(wgt).__name__, g, got, out)


def test_infeasible_budget(hip, orc):
    """no engine runs: CP_INFEASIBLE and the degenerate vector from both entries, whatever path the pair would have taken"""
    A = mat()
    f = cp.ConstrainedCost(CONN, PINS, int(A.nnz / K) - 50)
    for opts in ((), FORCE):
        with options(hip, opts):
            for order in ("splitter", "chunker"):
                got, out = path_of(hip, lambda: cp.partition_stripe(A, K, METHODS[(SUM, order)](f), backend=hip), constrained=True)
                assert got == ("OneWave" if opts else "None"), (opts, order, got)
                assert out.spl.tolist() == [1] * K + [A.n + 1] and out == cp.partition_stripe(A, K, METHODS[(SUM, order)](f), backend=orc)
    got, out = path_of(hip, lambda: tables_entry(hip, A, SUM, f), constrained=True)
    assert got == "None" and out[0] == M.CP_INFEASIBLE
    spl = np.zeros(K + 1, dtype=np.int64)
    assert hip.partition_dynamic(A, K, SUM, M.CP_ORDER_SPLITTER, CONN.marshal(), None, PINS.marshal(), int(A.nnz / K) - 50, 0.0, spl) == M.CP_INFEASIBLE
    assert spl.tolist() == [1] * K + [A.n + 1]
