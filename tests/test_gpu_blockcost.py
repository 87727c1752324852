"""BlockComponentCostModel as a weighted net count on the quotient pattern (csrc/blockcost.hip): cp.quotientpattern, the window
table + (min,+) scan behind DynamicTotalChunker(ConstrainedCost(block, VertexCount(), w <= 16)), the wave-per-query evaluation behind
oracle_stripe / total_value / bottleneck_value, their gate (blockcost_exact) and the option blockcost_par.  Every result is held
against the CPU oracle, against the stateful one-wave kernels (force_brute = 1, the path before this file) and, for the costs,
against the definition evaluated on the dense pattern."""
import numpy as np
import pytest

from util import cp, sprand, banded, suitesparse_shaped, golden_matrices, dense_mask

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 3, 5, 8, 16, 17)
EDGE_NS = (63, 64, 65, 129, 4097)             # the scan's blocks hold L = 64 rows


def small_matrices():
    rng = np.random.default_rng(23)
    out = {f"sprand{m}x{n}": sprand(m, n, 0.3, rng) for m, n in ((1, 1), (3, 5), (8, 16), (17, 9), (30, 65))}
    out["lpi_itest6"] = golden_matrices()["LPnetlib/lpi_itest6"]
    return out


def edge_matrix(kind, n):
    return banded(n, 5, 0.5, n) if kind == "banded" else suitesparse_shaped(n, 4, n)


MATRIX_IDS = list(small_matrices()) + [f"{kind}{n}" for n in EDGE_NS for kind in ("banded", "shaped")]
_cache = {}


def matrix(mid):
    if mid not in _cache:
        small = small_matrices()
        _cache[mid] = small[mid] if mid in small else edge_matrix("banded" if mid.startswith("banded") else "shaped",
                                                                   int(mid.lstrip("bandedshaped")))
    return _cache[mid]


def row_partitions(A):
    """name -> split of the rows of A: the EquiChunker packings of the adjoint, one part, and a split with empty parts"""
    T = cp.adjointpattern(A)
    out = {f"equi{u}": cp.pack_stripe(T, cp.EquiChunker(u)) for u in (1, 2, 4)}
    out["one"] = cp.SplitPartition(1, [1, A.m + 1])
    a, b = 1 + A.m // 3, 1 + (2 * A.m) // 3
    out["empty"] = cp.SplitPartition(6, [1, 1, a, a, b, A.m + 1, A.m + 1])
    return out


def models(A):
    """name -> (model, inside the gate).  The three models of test_gpu_chunkers.py::test_block_costs, their Float64 twins, two Float64
    models with non-integral entries (frac: tuple tables, which end at width 2 and part size 2 -- see in_domain; frac2: closures) and
    an Int64 model whose beta_col table holds 2^59 at width 0, where every count it multiplies is 0 (the gate's bound multiplies it
    by the weighted entries of the quotient pattern, at least 4: outside the gate unless the pattern is empty)."""
    out = {}
    for dt, tag in ((int, "i"), (float, "f")):
        out[tag + "0"] = (cp.BlockComponentCostModel(0, 0, (2, lambda x: x), (2, lambda x: 2 * x), dtype=dt), True)
        out[tag + "1"] = (cp.BlockComponentCostModel(lambda x: x, lambda x: 3 * x, (10, lambda x: x), (2, lambda x: 2 * x), dtype=dt), True)
        out[tag + "2"] = (cp.BlockComponentCostModel(1, 3, (1,), (1,), dtype=dt), True)
    out["frac"] = (cp.BlockComponentCostModel(1.5, (1, 2), (2, (3, 4.5)), (1, 1), dtype=float), False)
    out["frac2"] = (cp.BlockComponentCostModel(1.5, lambda w: 1 + w, (2, lambda u: 1.5 * u), (1, lambda w: w), dtype=float), False)
    out["big"] = (cp.BlockComponentCostModel(0, lambda w: w, (lambda u: 4 * u,), (lambda w: 2 ** 59 if w == 0 else 1 + w,)), A.nnz == 0)
    return out


def domain(mdl):
    """(largest width, largest part size) the model's tuple components hold -- f[w] past the tuple's end is a BoundsError in the
    reference and an error of the CPU oracle; None: closures and numbers, no limit"""
    wl = min((len(f) for f in (mdl.alpha_col, *mdl.beta_col) if isinstance(f, tuple)), default=None)
    ul = min((len(f) for f in mdl.beta_row if isinstance(f, tuple)), default=None)
    return wl, ul


def in_domain(mdl, Pi, w):
    wl, ul = domain(mdl)
    return (wl is None or w <= wl) and (ul is None or np.diff(Pi.spl).max() <= ul)


def chunker(mdl, w):
    return cp.DynamicTotalChunker(cp.ConstrainedCost(mdl, cp.VertexCount(), w))


class options:
    """with options(hip, name=value, ...): the options set, and back at their defaults (0 / 1) afterwards"""
    DEFAULTS = {"force_brute": 0, "blockcost_par": 1}

    def __init__(self, hip, **kv):
        self.hip, self.kv = hip, kv

    def __enter__(self):
        for k, v in self.kv.items():
            assert self.hip.set_option(k, v) == 0, k

    def __exit__(self, *exc):
        for k in self.kv:
            self.hip.set_option(k, self.DEFAULTS[k])


def packed(hip, A, mdl, w, Pi):
    """(split vector, blockcost_scan_packs of the call)"""
    hip.set_option("stat_reset", 0)
    P = cp.pack_stripe(A, chunker(mdl, w), Pi, backend=hip)
    return P, hip.get_stat("blockcost_scan_packs")


# ---------------------------------------------------------------- 1. the quotient pattern
@pytest.mark.parametrize("mid", MATRIX_IDS)
def test_quotient_pattern(hip, mid):
    A = matrix(mid)
    D = dense_mask(A)
    for name, Pi in row_partitions(A).items():
        Q = cp.quotientpattern(A, Pi, backend=hip)
        assert (Q.m, Q.n) == (Pi.K, A.n), (mid, name)
        for c in range(Q.n):
            assert np.all(np.diff(Q.rowval[Q.colptr[c] - 1:Q.colptr[c + 1] - 1]) > 0), (mid, name, c)
        want = np.array([D[Pi.spl[k] - 1:Pi.spl[k + 1] - 1].any(axis=0) for k in range(Pi.K)]).reshape(Pi.K, A.n)
        assert np.array_equal(dense_mask(Q), want), (mid, name)


def test_quotient_pattern_refuses_what_is_no_split(hip):
    A = matrix("sprand8x16")
    with pytest.raises(AssertionError, match="SplitPartition"):
        cp.quotientpattern(A, cp.MapPartition(2, [1, 2] * 4), backend=hip)
    with pytest.raises(AssertionError, match="does not cover"):
        cp.quotientpattern(A, cp.SplitPartition(2, [1, 4, 8]), backend=hip)


# ---------------------------------------------------------------- 2. chunker parity and the path taken
def check_chunker(hip, orc, A, Pi, mdl, inside, tag, brute=True):
    for w in (w for w in WIDTHS if in_domain(mdl, Pi, w)):
        got, packs = packed(hip, A, mdl, w, Pi)
        assert packs == (1 if inside and w <= 16 else 0), (tag, w, packs)
        assert np.all(np.diff(got.spl) <= w), (tag, w)
        assert got == cp.pack_stripe(A, chunker(mdl, w), Pi, backend=orc), (tag, w, "oracle")
        if brute:
            with options(hip, force_brute=1):
                lit, packs = packed(hip, A, mdl, w, Pi)
            assert packs == 0 and got == lit, (tag, w, "one-wave kernel")


@pytest.mark.parametrize("mid", [m for m in MATRIX_IDS if not m.endswith("4097")])
def test_chunker_parity_and_path(hip, orc, mid):
    """every matrix below the largest edge size x every row partition x every model x every width"""
    A = matrix(mid)
    for pname, Pi in row_partitions(A).items():
        for mname, (mdl, inside) in models(A).items():
            check_chunker(hip, orc, A, Pi, mdl, inside, (mid, pname, mname))


@pytest.mark.parametrize("mid", ["banded4097", "shaped4097"])
def test_chunker_parity_past_one_scan_block(hip, orc, mid):
    """n = 4097 (65 scan blocks): every partition for one model and every model for one partition against the oracle; the one-wave
    kernel walks n * w pairs on one lane, so it is held against three of those pairs only"""
    A = matrix(mid)
    parts, mdls = row_partitions(A), models(A)
    pairs = [(p, "i1") for p in parts] + [("equi2", m) for m in mdls if m != "i1"]
    for pname, mname in pairs:
        mdl, inside = mdls[mname]
        check_chunker(hip, orc, A, parts[pname], mdl, inside, (mid, pname, mname), brute=(pname, mname) in (("equi2", "i1"), ("empty", "i1"), ("equi2", "f0")))


def test_chunker_equals_one_wave_kernel_at_20000(hip):
    """the self-comparison only (the CPU oracle is out of reach), w in {3, 8, 16}"""
    A = suitesparse_shaped(20000, 4, 20000)
    Pi = cp.pack_stripe(cp.adjointpattern(A), cp.EquiChunker(4))
    mdls = models(A)
    for mname in ("i1", "f0"):
        for w in (3, 8, 16):
            got, packs = packed(hip, A, mdls[mname][0], w, Pi)
            assert packs == 1 and np.all(np.diff(got.spl) <= w)
            with options(hip, force_brute=1):
                lit, packs = packed(hip, A, mdls[mname][0], w, Pi)
            assert packs == 0 and got == lit, (mname, w)


@pytest.mark.parametrize("mid", ["sprand8x16", "lpi_itest6", "shaped65", "banded129"])
def test_option_blockcost_par_restores_the_one_wave_kernel(hip, orc, mid):
    A = matrix(mid)
    mdls = models(A)
    for pname, Pi in row_partitions(A).items():
        for mname in ("i0", "i1", "f2"):
            for w in (2, 8, 16):
                with options(hip, blockcost_par=0):
                    got, packs = packed(hip, A, mdls[mname][0], w, Pi)
                assert packs == 0 and got == cp.pack_stripe(A, chunker(mdls[mname][0], w), Pi, backend=orc), (mid, pname, mname, w)


@pytest.mark.parametrize("mid", MATRIX_IDS)
def test_pack_stripe_tables_on_both_paths(hip, mid):
    A = matrix(mid)
    Pi = row_partitions(A)["equi2"]
    mdls = models(A)
    for mname in (("i1",) if mid.endswith("4097") else ("i0", "i1", "i2", "f1")):
        for w in (w for w in WIDTHS if w <= 16):
            hip.set_option("stat_reset", 0)
            cst, spl = cp.pack_stripe_tables(A, chunker(mdls[mname][0], w), Pi, backend=hip)
            assert hip.get_stat("blockcost_scan_packs") == 1
            with options(hip, force_brute=1):
                cst0, spl0 = cp.pack_stripe_tables(A, chunker(mdls[mname][0], w), Pi, backend=hip)
            assert hip.get_stat("blockcost_scan_packs") == 1           # (the second call did not count)
            assert cst.dtype == cst0.dtype and np.array_equal(cst, cst0) and np.array_equal(spl, spl0), (mid, mname, w)


# ---------------------------------------------------------------- 3. Float64 inside the gate
@pytest.mark.parametrize("mid", MATRIX_IDS)
def test_integral_float_model_chunks_as_its_int_twin(hip, orc, mid):
    A = matrix(mid)
    mdls = models(A)
    for pname, Pi in row_partitions(A).items():
        for t in "012":
            for w in (3, 16):
                fi, packs = packed(hip, A, mdls["f" + t][0], w, Pi)
                assert packs == 1
                ii, packs = packed(hip, A, mdls["i" + t][0], w, Pi)
                assert packs == 1 and fi == ii, (mid, pname, t, w)
                assert fi == cp.pack_stripe(A, chunker(mdls["f" + t][0], w), Pi, backend=orc), (mid, pname, t, w)


# ---------------------------------------------------------------- 4. stateless evaluation
def definition(D, Pi, mdl, j, jp):
    """cost(j, j') = alpha_col(w) + sum_r d[r] * beta_col[r](w), d[r] = sum over the parts holding a nonzero of columns j .. j'-1 of
    beta_row[r](rows of the part), from the dense pattern"""
    fn = lambda f, x: f(x) if callable(f) else (f[min(x, len(f)) - 1] if x >= 1 else 0) if isinstance(f, tuple) else f
    w = jp - j
    below = np.concatenate([[0], np.cumsum(D[:, j - 1:jp - 1].any(axis=1))])          # touched rows among the first i
    hit = below[Pi.spl[1:] - 1] > below[Pi.spl[:-1] - 1]
    sizes = np.diff(Pi.spl)[hit]
    c = fn(mdl.alpha_col, w)
    for r in range(len(mdl.beta_row)):
        c += sum(fn(mdl.beta_row[r], int(u)) for u in sizes) * fn(mdl.beta_col[r], w)
    return c


def queries(n, rng, nq=200, wl=None):
    """wl: the widest query (a model whose tuple tables end there).  In the order of j': the one-wave kernel this is compared with
    rescans the pattern from column 1 whenever j' decreases (random orders: test_gpu_independent.py)"""
    js = rng.integers(1, n + 2, nq)
    jps = np.array([rng.integers(j, n + 2) for j in js])
    js[:4], jps[:4] = (1, 1, n + 1, max(1, n // 2)), (n + 1, 1, n + 1, n + 1)      # every column, j == j' at both ends, j' = n + 1
    if wl is not None:
        jps = np.minimum(jps, js + wl)
    order = np.lexsort((js, jps))
    return js[order].astype(np.int64), jps[order].astype(np.int64)


@pytest.mark.parametrize("mid", [m for m in MATRIX_IDS if not m.endswith("4097")] + ["banded4097"])
def test_wave_evaluation_equals_the_definition(hip, mid):
    A = matrix(mid)
    D = dense_mask(A)
    rng = np.random.default_rng(41)
    parts = row_partitions(A)
    mdls = models(A)
    for pname in (parts if A.n <= 129 else ("equi2",)):
        Pi = parts[pname]
        for mname in (mdls if A.n <= 129 else ("i1", "f0", "frac2")):
            mdl, inside = mdls[mname]
            if not in_domain(mdl, Pi, 0):
                continue
            js, jps = queries(A.n, rng, wl=domain(mdl)[0])
            hip.set_option("stat_reset", 0)
            got = cp.oracle_stripe(cp.StepHint(), mdl, A, Pi, backend=hip)(js, jps)
            assert hip.get_stat("blockcost_wave_evals") == (len(js) if inside else 0), (mid, pname, mname)
            with options(hip, force_brute=1):
                lit = cp.oracle_stripe(cp.StepHint(), mdl, A, Pi, backend=hip)(js, jps)
            assert hip.get_stat("blockcost_wave_evals") == (len(js) if inside else 0)
            assert got.dtype == lit.dtype and np.array_equal(got, lit), (mid, pname, mname)
            for t in range(len(js) if A.n <= 129 else 40):
                assert got[t] == definition(D, Pi, mdl, int(js[t]), int(jps[t])), (mid, pname, mname, js[t], jps[t])


def test_a_reversed_query_stays_on_the_step_oracle(hip):
    """one j > j' pair in the batch: no wave evaluation, and the answer of the one-wave kernel's driver (it refuses the batch)"""
    A = matrix("sprand8x16")
    Pi = row_partitions(A)["equi2"]
    mdl = models(A)["i1"][0]
    js, jps = queries(A.n, np.random.default_rng(5), 20)
    js[7], jps[7] = 9, 4
    said = []
    for brute in (0, 1):
        hip.set_option("stat_reset", 0)
        with options(hip, force_brute=brute):
            with pytest.raises(AssertionError) as e:
                cp.oracle_stripe(cp.StepHint(), mdl, A, Pi, backend=hip)(js, jps)
        said.append(str(e.value))
        assert hip.get_stat("blockcost_wave_evals") == 0
    assert said[0] == said[1] and "1 <= j <= j' <= n+1" in said[0]


@pytest.mark.parametrize("mid", [m for m in MATRIX_IDS if not m.endswith("4097")] + ["shaped4097"])
def test_objectives_take_one_wave_per_part(hip, orc, mid):
    A = matrix(mid)
    parts = row_partitions(A)
    for pname in (parts if A.n <= 129 else ("equi4",)):
        Pi = parts[pname]
        for mname, (mdl, inside) in models(A).items():
            for w in (w for w in (1, 2, 4) if in_domain(mdl, Pi, w)):
                Phi = cp.pack_stripe(A, cp.EquiChunker(w))
                for value in (cp.total_value, cp.bottleneck_value):
                    hip.set_option("stat_reset", 0)
                    got = value(A, Phi, mdl, Pi, backend=hip)
                    assert hip.get_stat("blockcost_wave_evals") == (Phi.K if inside else 0), (mid, pname, mname, w)
                    assert got == value(A, Phi, mdl, Pi, backend=orc), (mid, pname, mname, w, value.__name__)


# ---------------------------------------------------------------- 5. the 2-D pipeline
@pytest.mark.parametrize("mid", ["sprand1x1", "sprand30x65", "lpi_itest6", "banded63", "shaped64", "banded65", "shaped129", "banded4097"])
def test_pack_plaid_runs_its_block_chunkers_on_the_scan(hip, orc, mid):
    A = matrix(mid)
    for mname in ("i0", "i1", "f1"):
        mdl = models(A)[mname][0]
        packers = [cp.AlternatingPacker(cp.EquiChunker(2), chunker(mdl, 4), chunker(mdl, 3))]
        if A.m == A.n:
            packers.append(cp.SymmetricPacker(cp.EquiChunker(2), chunker(mdl, 4), chunker(mdl, 3)))
        for packer in packers:
            hip.set_option("stat_reset", 0)
            got = cp.pack_plaid(A, packer, backend=hip)
            assert hip.get_stat("blockcost_scan_packs") == 2, (mid, mname, type(packer).__name__)
            want = cp.pack_plaid(A, packer, backend=orc)
            assert got[0] == want[0] and got[1] == want[1], (mid, mname, type(packer).__name__)
