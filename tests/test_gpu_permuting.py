"""PermutingPartitioner(prm, prt) (reference src/PermutingPartitioner.jl) through its four entry points -- partition_stripe,
pack_stripe, partition_plaid, pack_plaid -- against the same steps composed by hand from permute_plaid, permute and the inner call,
and the pipeline of the reference's bottleneck script (bin/test_table_bottleneck.jl:49) on can_292."""
import numpy as np
import pytest

from util import cp, golden_matrices

gpu = pytest.mark.gpu

RCM = cp.CuthillMcKeePermuter()
NET = cp.AffineConnectivityModel(0, 10, 1, 100)
MATRICES = ("HB/can_292", "HB/west0132", "LPnetlib/lp_etamacro")


def covers_once(P, n):
    asg = cp.to_map(P).asg
    return asg.shape == (n,) and asg.min() >= 1 and asg.max() <= P.K and np.array_equal(np.sort(P.prm), np.arange(1, n + 1))


@gpu
@pytest.mark.parametrize("name", MATRICES)
def test_partition_stripe(hip, name):
    A = golden_matrices()[name]
    tau = cp.permute_stripe(A, RCM, backend=hip)
    B = cp.permute(A, None, tau, backend=hip)
    for K in (1, 3, 8):
        inner = cp.DynamicTotalSplitter(NET)
        got = cp.partition_stripe(A, K, cp.PermutingPartitioner(RCM, inner), backend=hip)
        want = tau[cp.partition_stripe(B, K, inner, backend=hip)]
        assert isinstance(got, cp.DomainPartition) and got == want and got.K == K and covers_once(got, A.n)
    # reversed and identity permuters
    got = cp.partition_stripe(A, 4, cp.PermutingPartitioner(cp.IdentityPermuter(), cp.DynamicTotalSplitter(NET)), backend=hip)
    assert got == cp.to_domain(cp.partition_stripe(A, 4, cp.DynamicTotalSplitter(NET), backend=hip))
    rev = cp.CuthillMcKeePermuter(reverse=True)
    got = cp.partition_stripe(A, 4, cp.PermutingPartitioner(rev, cp.DynamicTotalSplitter(NET)), backend=hip)
    tr = cp.permute_stripe(A, rev, backend=hip)
    assert np.array_equal(tr.prm, tau.prm[::-1])
    assert got == tr[cp.partition_stripe(cp.permute(A, None, tr, backend=hip), 4, cp.DynamicTotalSplitter(NET), backend=hip)]


@gpu
def test_partition_stripe_with_a_row_partition(hip):
    """PermutingPartitioner.jl:27-34: only the columns are permuted, the row partition passes through"""
    A = golden_matrices()["LPnetlib/lp_etamacro"]
    K = 4
    Pi = cp.partition_stripe(cp.adjointpattern(A, backend=hip), K, cp.EquiSplitter())
    inner = cp.DynamicTotalSplitter(cp.AffinePrimaryConnectivityModel(0, 10, 1, 100, 50))
    tau = cp.permute_stripe(A, RCM, backend=hip)
    B = cp.permute(A, None, tau, backend=hip)
    got = cp.partition_stripe(A, K, cp.PermutingPartitioner(RCM, inner), Pi, backend=hip)
    assert got == tau[cp.partition_stripe(B, K, inner, Pi, backend=hip)] and covers_once(got, A.n)


@gpu
@pytest.mark.parametrize("name", MATRICES)
def test_pack_stripe(hip, name):
    A = golden_matrices()[name]
    tau = cp.permute_stripe(A, RCM, backend=hip)
    B = cp.permute(A, None, tau, backend=hip)
    for inner in (cp.StrictChunker(4), cp.DynamicTotalChunker(cp.ConstrainedCost(NET, cp.VertexCount(), 9))):
        got = cp.pack_stripe(A, cp.PermutingPartitioner(RCM, inner), backend=hip)
        inner_res = cp.pack_stripe(B, inner, backend=hip)
        assert isinstance(got, cp.DomainPartition) and got == tau[inner_res] and got.K == inner_res.K and covers_once(got, A.n)


@gpu
@pytest.mark.parametrize("name", MATRICES)
def test_partition_plaid(hip, name):
    A = golden_matrices()[name]
    sigma, tau = cp.permute_plaid(A, RCM, backend=hip)
    B = cp.permute(A, sigma, tau, backend=hip)
    inner = cp.AlternatingPartitioner(cp.DynamicTotalSplitter(NET), cp.DynamicTotalSplitter(NET))
    for K in (2, 5):
        Pi, Phi = cp.partition_plaid(A, K, cp.PermutingPartitioner(RCM, inner), backend=hip)
        Pi_b, Phi_b = cp.partition_plaid(B, K, inner, backend=hip)
        assert Pi == sigma[Pi_b] and Phi == tau[Phi_b] and covers_once(Pi, A.m) and covers_once(Phi, A.n)
        # a caller's adjoint serves the ordering; the inner call works on the adjoint of B
        Pi2, Phi2 = cp.partition_plaid(A, K, cp.PermutingPartitioner(RCM, inner), adj_A=cp.adjointpattern(A, backend=hip), backend=hip)
        assert Pi2 == Pi and Phi2 == Phi


@gpu
@pytest.mark.parametrize("name", MATRICES)
def test_pack_plaid(hip, name):
    A = golden_matrices()[name]
    sigma, tau = cp.permute_plaid(A, RCM, backend=hip)
    B = cp.permute(A, sigma, tau, backend=hip)
    inner = cp.AlternatingPacker(cp.StrictChunker(4), cp.StrictChunker(6))
    Pi, Phi = cp.pack_plaid(A, cp.PermutingPartitioner(RCM, inner), backend=hip)
    Pi_b, Phi_b = cp.pack_plaid(B, inner, backend=hip)
    assert Pi == sigma[Pi_b] and Phi == tau[Phi_b] and covers_once(Pi, A.m) and covers_once(Phi, A.n)


@gpu
@pytest.mark.parametrize("K", (2, 4))
def test_script_pipeline_on_can_292(hip, K):
    """bin/test_table_bottleneck.jl:22, :49"""
    A = golden_matrices()["HB/can_292"]
    sym_model = cp.AffineMonotonizedSymmetricConnectivityModel(0, 0, 1, 100, 90)
    method = cp.PermutingPartitioner(cp.CuthillMcKeePermuter(), cp.SymmetricPartitioner(cp.LazyBisectCostBottleneckSplitter(sym_model, 0.01)))
    Pi, Phi = cp.partition_plaid(A, K, method, backend=hip)
    assert isinstance(Pi, cp.DomainPartition) and Pi == Phi and Pi.K == K
    for P in (Pi, Phi):
        asg = cp.to_map(P).asg
        assert np.array_equal(np.sort(P.prm), np.arange(1, A.n + 1)) and asg.min() >= 1 and asg.max() <= K
        assert np.array_equal(np.bincount(asg, minlength=K + 1)[1:], np.diff(P.spl))
    # the same steps by hand
    sigma, tau = cp.permute_plaid(A, cp.CuthillMcKeePermuter(), backend=hip)
    assert sigma is tau
    Pi_b, Phi_b = cp.partition_plaid(cp.permute(A, sigma, tau, backend=hip), K, method.prt, backend=hip)
    assert Pi == sigma[Pi_b] and Phi == tau[Phi_b]


@gpu
def test_other_methods_still_refused(hip):
    A = golden_matrices()["HB/can_292"]
    with pytest.raises(NotImplementedError):
        cp.partition_plaid(A, 2, cp.PermutingPartitioner(object(), cp.SymmetricPartitioner(cp.EquiSplitter())), backend=hip)
