"""total_value / bottleneck_value of non-contiguous column partitions (compute_objective for any Phi, reference src/Costs.jl:34-39,
:52-57): against the definition of every part's cost on a dense mask, Map and Domain forms alike, and the results of
PermutingPartitioner against their permuted twins."""
import numpy as np
import pytest

import map_model as mm
from util import cp, golden_matrices

gpu = pytest.mark.gpu
MATRICES = ("HB/can_292", "HB/west0132", "LPnetlib/lp_etamacro")
# Int64 models, and a Float64 one whose parameters are dyadic: every cost and every sum is exact in any order
MODELS = (cp.AffineWorkModel(3, 10, 1), cp.AffineConnectivityModel(1, 10, 1, 100), cp.AffineHyperedgeCutModel(2, 10, 1, 7, 100),
          cp.AffineConnectivityModel(0.5, 0.25, 1.5, 2.75), cp.AffineConnectivityModel(0, 3, 1, 3, alpha_k=[5, 0, 9]))
RCM = cp.CuthillMcKeePermuter()


def values(A, Phi, mdl, Pi=None, **kw):
    return cp.total_value(A, Phi, mdl, Pi, **kw), cp.bottleneck_value(A, Phi, mdl, Pi, **kw)


def from_definition(A, Phi, mdl, Pi=None):
    costs = mm.part_costs(A, Phi, mdl, Pi)
    total = 0 if mdl.dtype == 0 else 0.0
    for c in costs:
        total = total + c
    return total, max(costs)


@gpu
@pytest.mark.parametrize("name", MATRICES)
def test_map_partitions_score_as_defined(hip, name):
    A = golden_matrices()[name]
    rng = np.random.default_rng(A.n)
    cases = [(3, rng.integers(1, 4, A.n)), (7, rng.integers(1, 8, A.n)),
             (9, rng.choice([2, 5, 9], A.n)),                           # parts 1, 3, 4, 6, 7, 8 are empty
             (A.n + 10, rng.permutation(A.n + 10)[:A.n] + 1),            # K > n: every part holds at most one column
             (1, np.ones(A.n, dtype=np.int64))]
    for K, asg in cases:
        Phi = cp.MapPartition(K, asg)
        dom = cp.to_domain(Phi)
        scrambled = cp.DomainPartition(K, np.concatenate([rng.permutation(dom.prm[a - 1:b - 1]) for a, b in zip(dom.spl[:-1], dom.spl[1:])]), dom.spl)
        for mdl in MODELS if K != 1 else MODELS[:3]:
            if mdl.alpha_k is not None and K > len(mdl.alpha_k):
                continue
            want = from_definition(A, Phi, mdl)
            for P in (Phi, dom, scrambled):
                got = values(A, P, mdl, backend=hip)
                assert got == want, (name, K, type(mdl).__name__, got, want)


@gpu
def test_map_partition_under_a_primary_model(hip):
    """Pi, a partition of the rows, passes through the column gather unchanged, whatever its kind"""
    A = golden_matrices()["LPnetlib/lp_etamacro"]
    K = 5
    rng = np.random.default_rng(1)
    comm = cp.AffinePrimaryConnectivityModel(0, 10, 1, 0, 100)
    Phi = cp.MapPartition(K, rng.integers(1, K + 1, A.n))
    for Pi in (cp.MapPartition(K, rng.integers(1, K + 1, A.m)), cp.partition_stripe(cp.adjointpattern(A, backend=hip), K, cp.EquiSplitter())):
        want = from_definition(A, Phi, comm, Pi)
        for P in (Phi, cp.to_domain(Phi)):
            for row_form in (Pi, cp.to_domain(Pi)):
                assert values(A, P, comm, row_form, backend=hip) == want


@gpu
def test_split_partitions_score_as_before(hip):
    A = golden_matrices()["HB/west0132"]
    for mdl in MODELS[:4]:
        for K in (1, 4, 9):
            Phi = cp.partition_stripe(A, K, cp.EquiSplitter())
            got = values(A, Phi, mdl, backend=hip)
            assert got == from_definition(A, Phi, mdl)
            assert got == values(A, cp.to_map(Phi), mdl, backend=hip) == values(A, cp.to_domain(Phi), mdl, backend=hip)


@gpu
@pytest.mark.parametrize("name", MATRICES)
def test_permuted_results_score_like_their_twins(hip, name):
    A = golden_matrices()[name]
    net = cp.AffineConnectivityModel(0, 10, 1, 100)
    comm = cp.AffinePrimaryConnectivityModel(0, 10, 1, 0, 100)
    K = 4
    # stripe: value(A, tau[Phi_b]) == value(permute(A, None, tau), Phi_b)
    tau = cp.permute_stripe(A, RCM, backend=hip)
    B = cp.permute(A, None, tau, backend=hip)
    Phi_b = cp.partition_stripe(B, K, cp.DynamicTotalSplitter(net), backend=hip)
    Phi = cp.partition_stripe(A, K, cp.PermutingPartitioner(RCM, cp.DynamicTotalSplitter(net)), backend=hip)
    assert isinstance(Phi, cp.DomainPartition) and Phi == tau[Phi_b]
    for mdl in MODELS[:3]:
        assert values(A, Phi, mdl, backend=hip) == values(B, Phi_b, mdl, backend=hip) == from_definition(A, Phi, mdl)
    # plaid with a primary model: value(A, tau[Phi_b], comm, Pi = sigma[Pi_b]) == value(B, Phi_b, comm, Pi = Pi_b)
    sigma, tau = cp.permute_plaid(A, RCM, backend=hip)
    B = cp.permute(A, sigma, tau, backend=hip)
    inner = cp.AlternatingPartitioner(cp.DynamicTotalSplitter(net), cp.DynamicTotalSplitter(net))
    Pi_b, Phi_b = cp.partition_plaid(B, K, inner, backend=hip)
    Pi, Phi = cp.partition_plaid(A, K, cp.PermutingPartitioner(RCM, inner), backend=hip)
    assert Pi == sigma[Pi_b] and Phi == tau[Phi_b]
    got = values(A, Phi, comm, Pi, backend=hip)
    assert got == values(B, Phi_b, comm, Pi_b, backend=hip) == from_definition(A, Phi, comm, Pi)


@gpu
@pytest.mark.parametrize("K", (2, 4))
def test_script_pipeline_scores_on_can_292(hip, K):
    """bin/test_table_bottleneck.jl:49 with its score: the symmetric cost of sigma[Pi_b] on A is that of Pi_b on permute(A, sigma,
    sigma) -- one partition for rows and columns, so both sides are gathered"""
    A = golden_matrices()["HB/can_292"]
    sym_model = cp.AffineMonotonizedSymmetricConnectivityModel(0, 0, 1, 100, 90)
    method = cp.PermutingPartitioner(RCM, cp.SymmetricPartitioner(cp.LazyBisectCostBottleneckSplitter(sym_model, 0.1)))
    Pi, Phi = cp.partition_plaid(A, K, method, backend=hip)
    sigma, tau = cp.permute_plaid(A, RCM, backend=hip)
    assert sigma is tau
    B = cp.permute(A, sigma, sigma, backend=hip)
    Pi_b, _ = cp.partition_plaid(B, K, method.prt, backend=hip)
    assert Pi == sigma[Pi_b]
    for mdl in (sym_model, cp.AffineSymmetricConnectivityModel(0, 10, 1, 0, 100), cp.AffineSymmetricEdgeCutModel(0, 10, 1, 100)):
        assert values(A, Pi, mdl, backend=hip) == values(B, Pi_b, mdl, backend=hip)
        assert values(A, cp.to_map(Pi), mdl, backend=hip) == values(B, Pi_b, mdl, backend=hip)


@gpu
def test_secondary_model_still_needs_a_split_of_the_rows(hip):
    A = golden_matrices()["HB/west0132"]
    K = 3
    loc = cp.AffineSecondaryConnectivityModel(0, 10, 1, 0, 100)
    Phi = cp.partition_stripe(A, K, cp.EquiSplitter())
    Pi = cp.partition_stripe(cp.adjointpattern(A, backend=hip), K, cp.EquiSplitter())
    assert cp.total_value(A, Phi, loc, Pi, backend=hip) > 0
    for P in (cp.to_map(Pi), cp.to_domain(Pi)):
        for Phi_form in (Phi, cp.to_map(Phi)):
            with pytest.raises(AssertionError):
                cp.total_value(A, Phi_form, loc, P, backend=hip)
