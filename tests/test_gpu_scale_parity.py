"""Oracle parity at production size.

test_gpu_fullsize.py and bench.py check the full-size runs through the library's own counting structures (objective, bounds,
BisectIndex), so a wrong net or self-net count would move both sides of a comparison together.  Here the patterns are
generated on the device once, copied to the host once, and every count, model value, objective and split vector is
refereed by the CPU oracle (its NoHint structures) -- at the bench shape, the config-2 shape, and at mid-size shapes built to
hit the edges of the counter builds (hot rows, huge columns, empty runs, nnz around multiples of the 2048-key blocks, heights
around 2^20).
"""
import numpy as np
import pytest
import torch

from util import cp

pytestmark = pytest.mark.gpu

NOHINT = cp.NoHint()
HINTS = [cp.NoHint(), cp.RandomHint(), cp.SparseHint(), cp.StepHint()]


def host_pattern(n, N, seed):
    from bench import gen_suitesparse_shaped
    colptr, rowval = gen_suitesparse_shaped(n, N, seed, torch.device("cuda", 0))
    A = cp.SparseMatrixCSC(n, n, colptr.cpu().numpy(), rowval.cpu().numpy())
    del colptr, rowval
    torch.cuda.empty_cache()
    return A


def pattern(m, n, cols, rows):
    """CSC pattern from 0-based (col, row) entries; duplicates dropped, rows sorted inside each column"""
    key = np.unique(cols.astype(np.int64) * (m + 1) + rows.astype(np.int64))
    c, r = key // (m + 1), key % (m + 1)
    colptr = np.concatenate([[1], 1 + np.cumsum(np.bincount(c, minlength=n))]).astype(np.int64)
    return cp.SparseMatrixCSC(m, n, colptr, (r + 1).astype(np.int64))


def pairs(A, rng, nrand):
    """(j, j') query pairs: random, the whole range, j = j', widths 1, 2, 63, 64, 65 and 2^k +- 1, and the columns where colptr
    crosses a multiple of 64 and of 2048 (the 8-keys-per-thread x 256-thread block of the wavelet build)"""
    n = A.n
    j = rng.integers(1, n + 2, nrand); jp = rng.integers(1, n + 2, nrand)
    j, jp = np.minimum(j, jp), np.maximum(j, jp)
    L = [(1, n + 1), (1, 1), (n + 1, n + 1), (1, 2), (n, n + 1)]
    widths = [1, 2, 63, 64, 65] + [w for k in range(2, 24) for w in (2 ** k - 1, 2 ** k + 1)]
    starts = rng.integers(1, n + 2, 6).tolist()
    for blk in (64, 2048):
        pos = A.colptr - 1
        cross = np.nonzero(np.diff(pos // blk) > 0)[0] + 1           # columns (1-based) whose colptr entry passes a block boundary
        if cross.size:
            starts += rng.choice(cross, min(cross.size, 20), replace=False).tolist()
    for s in [1, n + 1] + starts:
        for w in widths:
            if s + w <= n + 1:
                L.append((s, s + w))
            if s - w >= 1:
                L.append((s - w, s))
        L.append((s, s))
    a = np.concatenate([j, np.array([p[0] for p in L], dtype=np.int64)])
    b = np.concatenate([jp, np.array([p[1] for p in L], dtype=np.int64)])
    return a, b


def dom_points(A, rng, nrand):
    m, n = A.m, A.n
    i = rng.integers(1, m + 2, nrand); j = rng.integers(1, n + 2, nrand)
    rows = [1, 2, m, m + 1] + [2 ** k for k in range(1, 40) if 2 ** k <= m + 1]
    cols = [1, 2, n, n + 1] + rng.integers(1, n + 2, 8).tolist()
    ii = np.array([r for r in rows for _ in cols], dtype=np.int64); jj = np.array([c for _ in rows for c in cols], dtype=np.int64)
    return np.concatenate([i, ii]), np.concatenate([j, jj])


def check_counts(hip, orc, A, rng, nrand=20000):
    """net / self-net / dominance counts of the device against the oracle's NoHint structures; returns the oracle's counts"""
    a, b = pairs(A, rng, nrand)
    want = {}
    for kind, count in (("net", cp.netcount), ("selfnet", cp.selfnetcount)):
        want[kind] = count(A, NOHINT, backend=orc)(a, b)
        for hint in HINTS:
            got = count(A, hint, backend=hip)(a, b)
            bad = np.nonzero(got != want[kind])[0]
            assert bad.size == 0, (kind, type(hint).__name__, A, a[bad[:5]], b[bad[:5]], got[bad[:5]], want[kind][bad[:5]])
    i, j = dom_points(A, rng, nrand // 4)
    dw = cp.dominancecount(A, NOHINT, backend=orc)(i, j)
    dg = cp.dominancecount(A, backend=hip)(i, j)
    bad = np.nonzero(dg != dw)[0]
    assert bad.size == 0, ("dom", A, i[bad[:5]], j[bad[:5]], dg[bad[:5]], dw[bad[:5]])
    return a, b, want["net"], want["selfnet"]


def model_values(mdl, A, j, jp, nn, nl, k):
    """the model applied to the oracle's counts, left to right in the model's element type (the reference's evaluation order)"""
    dt = np.int64 if mdl.dtype == cp.models.CP_I64 else np.float64
    pos = A.colptr - 1
    nv, npins = (jp - j).astype(dt), (pos[jp - 1] - pos[j - 1]).astype(dt)
    a = np.full(j.size, mdl.alpha, dtype=dt)
    if getattr(mdl, "alpha_k", None) is not None:
        ak = np.asarray(mdl.alpha_k, dtype=dt)
        inside = (k >= 1) & (k <= ak.size)
        a[inside] = ak[k[inside] - 1]
    v = a + nv * dt(mdl.beta_vertex) + npins * dt(mdl.beta_pin)
    if mdl.kind == cp.models.CP_MODEL_CONNECTIVITY:
        v = v + nn.astype(dt) * dt(mdl.beta_net)
    elif mdl.kind == cp.models.CP_MODEL_HYPEREDGE_CUT:
        v = v + nl.astype(dt) * dt(mdl.beta_self_net) + (nn - nl).astype(dt) * dt(mdl.beta_cut_net)
    return v


def check_model_values(hip, A, a, b, nn, nl, rng):
    k = rng.integers(1, 9, a.size)
    for mdl in (cp.AffineWorkModel(3, 10, 1), cp.AffineConnectivityModel(0, 10, 1, 100), cp.AffineHyperedgeCutModel(1, 2, 1, 3, 7),
                cp.AffineConnectivityModel(1.0, 10.0, 1.0, 100.0, alpha_k=[5.0, 1.0, 9.0, 2.0, 7.0, 3.0])):
        want = model_values(mdl, A, a, b, nn, nl, k)
        for hint in HINTS:
            out = np.zeros(a.size, dtype=want.dtype)
            assert hip.oracle_eval(A, mdl.marshal(), None, hint.code, a, b, k, out) == 0, hip.last_error()
            assert np.array_equal(out, want), (mdl.kind, type(hint).__name__)


def random_splits(rng, n, K, count):
    out = []
    for _ in range(count):
        s = np.sort(rng.integers(1, n + 2, K - 1))
        out.append(cp.SplitPartition(K, np.concatenate([[1], s, [n + 1]]).astype(np.int64)))
    return out


def check_objectives(hip, orc, A, splits, models):
    for mdl in models:
        for P in splits:
            for f in (cp.total_value, cp.bottleneck_value):
                assert f(A, P, mdl, backend=hip) == f(A, P, mdl, backend=orc), (f.__name__, mdl._params(), P)


def check_bottleneck_optimum(hip, orc, A, K, mdl):
    """the device bottleneck DP is optimal by the ORACLE's measure: its oracle bottleneck equals the oracle's BisectIndex
    optimum; the device BisectIndex split is the oracle's"""
    bi = cp.partition_stripe(A, K, cp.BisectIndexBottleneckSplitter(mdl), backend=orc)
    assert cp.partition_stripe(A, K, cp.BisectIndexBottleneckSplitter(mdl), backend=hip) == bi
    dp = cp.partition_stripe(A, K, cp.DynamicBottleneckSplitter(mdl), backend=hip)
    assert cp.bottleneck_value(A, dp, mdl, backend=orc) == cp.bottleneck_value(A, bi, mdl, backend=orc)
    return dp


def test_bench_shape_counts_objectives_and_optima_against_the_oracle(hip, orc):
    n, N = 10_000_000, 100_000_000
    A = host_pattern(n, N, 0xDEADBEEF + 2)
    rng = np.random.default_rng(1)
    a, b, nn, nl = check_counts(hip, orc, A, rng)
    check_model_values(hip, A, a, b, nn, nl, rng)
    conn = cp.AffineConnectivityModel(0, 10, 1, 100)
    dp = check_bottleneck_optimum(hip, orc, A, 16, conn)
    w = -(-3 * n // (2 * 16))
    constrained = cp.partition_stripe(A, 16, cp.DynamicTotalSplitter(cp.ConstrainedCost(conn, cp.VertexCount(), w)), backend=hip)
    check_objectives(hip, orc, A, random_splits(rng, n, 16, 1) + [dp, constrained], [conn])
    check_objectives(hip, orc, A, random_splits(rng, n, 7, 1), [cp.AffineHyperedgeCutModel(0, 0, 0, 0, 1)])
    assert cp.bound_stripe(A, 16, conn, backend=hip) == cp.bound_stripe(A, 16, conn, backend=orc)
    assert np.array_equal(hip.link_array(A), orc.link_array(A))


def test_config2_shape_bisect_cost_and_batch_against_the_oracle(hip, orc):
    n = 1_000_000
    A = host_pattern(n, 13 * n, 0xDEADBEEF + 1)
    for mdl in (cp.AffineWorkModel(0, 10, 1), cp.AffineConnectivityModel(0, 10, 1, 100)):
        meth = cp.BisectCostBottleneckSplitter(mdl, 0.01)
        assert cp.partition_stripe(A, 32, meth, backend=hip) == cp.partition_stripe(A, 32, meth, backend=orc), mdl._params()
    reqs = []
    for i, K in enumerate((2, 3, 5, 8, 13, 16, 21, 32, 33, 47, 64, 100, 128, 200, 255, 256)):
        mdl = (cp.AffineWorkModel(0, 10, 1), cp.AffineConnectivityModel(0, 10, 1, 100), cp.AffineConnectivityModel(3, 0, 1, 7))[i % 3]
        reqs.append((K, (cp.FlipBisectCostBottleneckSplitter if i % 5 == 4 and i % 3 else cp.BisectCostBottleneckSplitter)(mdl, (0.1, 0.01, 0.001)[i % 3])))
    got = cp.partition_stripe_batch(A, reqs, backend=hip)
    for (K, m), g in zip(reqs, got):
        assert g == cp.partition_stripe(A, K, m, backend=orc), (K, type(m).__name__, m.eps)
    rng = np.random.default_rng(3)
    asg = rng.integers(1, 33, A.m)
    g, w = hip.partwise(A, 32, asg), orc.partwise(A, 32, asg)
    assert g[0] == w[0] and all(np.array_equal(x, y) for x, y in zip(g[1:], w[1:]))


def edge_shapes():
    rng = np.random.default_rng(2024)
    out = {}
    # rectangular, tall (m = 8n) and flat (m = n/16)
    n = 300_000
    c = rng.integers(0, n, 3_000_000); out["tall"] = pattern(8 * n, n, c, rng.integers(0, 8 * n, c.size))
    c = rng.integers(0, n, 2_000_000); out["flat"] = pattern(n // 16, n, c, rng.integers(0, n // 16, c.size))
    # one row in every column (the longest net chain, the hot key of the histogram), one column of 2e5 entries,
    # 1e4 consecutive empty columns and empty rows (rows 5e5 .. m-1 never hit)
    n, m = 400_000, 600_000
    c = rng.integers(0, n, 2_000_000); r = rng.integers(0, 500_000, c.size)
    keep = (c < 100_000) | (c >= 110_000)
    c, r = c[keep], r[keep]
    c = np.concatenate([c, np.arange(n), np.full(200_000, 7777)]); r = np.concatenate([r, np.full(n, 12345), np.arange(200_000) * 2])
    keep = (c < 100_000) | (c >= 110_000)
    out["hot_row_huge_col_empty_run"] = pattern(m, n, c[keep], r[keep])
    # nnz = 0
    out["empty"] = cp.SparseMatrixCSC(1000, 1_000_000, np.ones(1_000_001, dtype=np.int64), np.zeros(0, dtype=np.int64))
    # nnz = 0, 1, 2047 (mod 2048) and m + 1 / n + 1 on both sides of 2^20
    for name, (m, n, resid) in {"h20_lo": (2 ** 20 - 2, 2 ** 20 - 2, 0), "h20_hi": (2 ** 20, 2 ** 20, 1), "h20_mix": (2 ** 20 - 1, 2 ** 20 + 1, 2047)}.items():
        c = rng.integers(0, n, 2_600_000); A = pattern(m, n, c, rng.integers(0, m, c.size))
        cut = A.nnz - ((A.nnz - resid) % 2048)                       # trim the last entries to the wanted residue
        colptr = np.minimum(A.colptr, cut + 1)
        out[name] = cp.SparseMatrixCSC(m, n, colptr, A.rowval[:cut])
        assert out[name].nnz % 2048 == resid
    return out


@pytest.mark.parametrize("name", ["tall", "flat", "hot_row_huge_col_empty_run", "empty", "h20_lo", "h20_hi", "h20_mix"])
def test_edge_shapes_against_the_oracle(hip, orc, name):
    A = edge_shapes_cache()[name]
    rng = np.random.default_rng(len(name))
    check_counts(hip, orc, A, rng, nrand=5000)
    conn = cp.AffineConnectivityModel(0, 10, 1, 100)
    hyp = cp.AffineHyperedgeCutModel(0, 2, 1, 1, 3)
    dp = check_bottleneck_optimum(hip, orc, A, 8, conn)
    check_objectives(hip, orc, A, random_splits(rng, A.n, 8, 1) + [dp], [conn, hyp])


def test_fast_tables_equal_the_literal_sweep_on_a_hot_row_shape(hip):
    """n <= 2e5: the complete fast tables against the force_brute device sweep on a pattern with a row in every column, a
    column of 5e4 entries and an empty run"""
    rng = np.random.default_rng(77)
    n, m = 60_000, 90_000
    c = rng.integers(0, n, 300_000); r = rng.integers(0, 80_000, c.size)
    c = np.concatenate([c, np.arange(n), np.full(50_000, 4321)]); r = np.concatenate([r, np.full(n, 99), np.arange(50_000)])
    keep = (c < 20_000) | (c >= 30_000)
    A = pattern(m, n, c[keep], r[keep])
    for mdl in (cp.AffineConnectivityModel(0, 10, 1, 100), cp.AffineHyperedgeCutModel(0, 2, 1, 1, 3)):
        mm = mdl.marshal()
        rc1, p1, c1 = hip.dynamic_tables(A, 3, 0, mm, None)
        hip.set_option("force_brute", 1)
        try:
            rc2, p2, c2 = hip.dynamic_tables(A, 3, 0, mm, None)
        finally:
            hip.set_option("force_brute", 0)
        assert rc1 == 0 and rc2 == 0, hip.last_error()
        assert np.array_equal(p1, p2) and np.array_equal(c1, c2), mdl._params()


_EDGE = {}


def edge_shapes_cache():
    if not _EDGE:
        _EDGE.update(edge_shapes())
    return _EDGE
