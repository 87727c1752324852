"""MagneticPartitioner and GreedyBottleneckPartitioner on the device (csrc/map_part.hip) against the loops of the reference
(tests/map_model.py), bit for bit: assignments, the visiting order and the final part costs, with the walk's state in LDS and in
global memory; the preconditions as status returns; and the callers -- partition_plaid chains and PermutingPartitioner."""
import numpy as np
import pytest

import map_model as mm
from greedy_model import from_columns
from util import cp, golden_matrices

gpu = pytest.mark.gpu
draws = cp.draws
LDS_DEFAULT = 2048


def greedy_both(hip, A, K, method, Pi):
    """the partition under the default option and with the walk's state in global memory: -> [(asg, order, cst)] * 2"""
    out = []
    try:
        for parts in (LDS_DEFAULT, 0):
            assert hip.set_option("greedy_lds_parts", parts) == 0
            P = cp.partition_stripe(A, K, method, Pi, backend=hip)
            assert isinstance(P, cp.MapPartition) and P.K == K and P.asg.shape == (A.n,)
            out.append((P.asg, hip.last_greedy["order"], hip.last_greedy["cst"]))
    finally:
        hip.set_option("greedy_lds_parts", LDS_DEFAULT)
    return out


def check_greedy(hip, A, T, K, Pi, mdl, seed, explicit):
    n = A.n
    if explicit:
        order = np.random.default_rng(seed).permutation(n).astype(np.int64) + 1
        method = cp.GreedyBottleneckPartitioner(mdl, order=order)
    else:
        order = draws.greedy_order(seed, n)
        method = cp.GreedyBottleneckPartitioner(mdl, seed=seed)
    asg, cst = mm.greedy(A, K, Pi, mdl, order, adj_A=T)
    for got_asg, got_order, got_cst in greedy_both(hip, A, K, method, Pi):
        assert np.array_equal(got_order, order)
        assert np.array_equal(got_asg, asg), (A, K, seed)
        assert got_cst.dtype == cst.dtype and got_cst.tobytes() == cst.tobytes(), (A, K, seed, got_cst, cst)


@gpu
@pytest.mark.parametrize("shape", mm.SHAPES)
def test_magnetic(hip, shape):
    m, density = shape
    rng = np.random.default_rng(m)
    for n in mm.NS:
        A, _ = mm.matrix(m, density, n)
        for K in mm.KS:
            for kind in ("split", "map"):
                Pi = mm.row_partition(kind, m, K)
                u = rng.integers(0, 2**63 - 1, n)
                got = cp.partition_stripe(A, K, cp.MagneticPartitioner(draws=u), Pi, backend=hip)
                assert isinstance(got, cp.MapPartition) and got.K == K and np.array_equal(got.asg, mm.magnetic(A, K, Pi, u))
                seed = 1000 * n + K
                got = cp.partition_stripe(A, K, cp.MagneticPartitioner(seed), Pi, backend=hip)
                assert np.array_equal(got.asg, mm.magnetic(A, K, Pi, draws.magnetic_draws(seed, n)))


@gpu
@pytest.mark.parametrize("K", mm.KS)
@pytest.mark.parametrize("shape", mm.SHAPES)
def test_greedy(hip, shape, K):
    """every size, both kinds of Pi, every model, the order given and from a seed"""
    m, density = shape
    for a, n in enumerate(mm.NS):
        A, T = mm.matrix(m, density, n)
        for kind in ("split", "map"):
            Pi = mm.row_partition(kind, m, K)
            for c, mdl in enumerate(mm.models(K)):
                for explicit in (True, False):
                    check_greedy(hip, A, T, K, Pi, mdl, seed=10 * a + c, explicit=explicit)


@gpu
def test_domain_row_partition(hip):
    m, density = mm.SHAPES[1]
    A, T = mm.matrix(m, density, 257)
    for K in (5, 64):
        Pi = mm.row_partition("domain", m, K)
        assert isinstance(Pi, cp.DomainPartition)
        check_greedy(hip, A, T, K, Pi, mm.models(K)[2], seed=K, explicit=False)
        got = cp.partition_stripe(A, K, cp.MagneticPartitioner(K), Pi, backend=hip)
        assert np.array_equal(got.asg, mm.magnetic(A, K, Pi, draws.magnetic_draws(K, A.n)))


@gpu
def test_both_sides_of_the_lds_bound(hip):
    """K = 2048 is the last K whose walk state fits LDS under the default option; 2049 walks in global memory"""
    m, density = mm.SHAPES[2]
    A, T = mm.matrix(m, density, 257)
    for K in (LDS_DEFAULT, LDS_DEFAULT + 1):
        for kind in ("split", "map"):
            check_greedy(hip, A, T, K, mm.row_partition(kind, m, K), mm.models(K)[3], seed=K, explicit=False)


@gpu
def test_special_shapes(hip):
    from greedy_model import transpose
    m = 70
    empty = from_columns(m, [np.zeros(0, dtype=np.int64)] * 9)
    one = from_columns(m, [np.arange(m, dtype=np.int64)])
    wide = from_columns(m, [np.arange(m, dtype=np.int64)] + [np.array([j, (7 * j) % m][:1 + j % 2], dtype=np.int64) for j in range(1, 6)])
    for A in (empty, one, wide):
        T = transpose(A)
        for K, Pi in ((3, mm.row_partition("split", m, 3)), (3, cp.MapPartition(3, np.full(m, 2, dtype=np.int64))),      # all rows in one part
                      (64, mm.row_partition("map", m, 64)), (300, mm.row_partition("split", m, 300))):                   # K > n
            for c in range(4):
                check_greedy(hip, A, T, K, Pi, mm.models(K)[c], seed=c, explicit=c % 2 == 0)
            u = draws.magnetic_draws(K, A.n)
            got = cp.partition_stripe(A, K, cp.MagneticPartitioner(K), Pi, backend=hip)
            assert np.array_equal(got.asg, mm.magnetic(A, K, Pi, u))
    got = cp.partition_stripe(empty, 7, cp.MagneticPartitioner(draws=np.arange(9)), mm.row_partition("map", m, 7), backend=hip)
    assert got.asg.tolist() == [1 + j % 7 for j in range(9)]


@gpu
@pytest.mark.parametrize("name", ["LPnetlib/lp_etamacro", "HB/can_292"])
def test_embedded_matrices(hip, name):
    """test/runbenchmarks.jl:48, :67-76: K = 2 and ceil(n^(3/4)); Pi the EquiSplitter split of the adjoint and mod1.(1:m, K)"""
    A = golden_matrices()[name]
    T = cp.adjointpattern(A, backend=hip)
    local_model = cp.AffineSecondaryConnectivityModel(0, 10, 1, 0, 100)
    for K in (2, int(np.ceil(A.n ** 0.75))):
        for Pi in (cp.partition_stripe(T, K, cp.EquiSplitter()), cp.MapPartition(K, np.arange(A.m) % K + 1)):
            check_greedy(hip, A, T, K, Pi, local_model, seed=K, explicit=False)
            got = cp.partition_stripe(A, K, cp.MagneticPartitioner(K), Pi, backend=hip)
            assert np.array_equal(got.asg, mm.magnetic(A, K, Pi, draws.magnetic_draws(K, A.n)))


@gpu
def test_preconditions_are_status_returns(hip):
    m, density = mm.SHAPES[1]
    A, _ = mm.matrix(m, density, 65)
    n, K = A.n, 5
    Pi = mm.row_partition("map", m, K)
    mdl = mm.models(K)[0]
    repeat = np.arange(1, n + 1)
    repeat[3] = repeat[9]
    beyond = np.arange(1, n + 1)
    beyond[0] = n + 1
    for order in (repeat, beyond, np.zeros(n, dtype=np.int64)):
        with pytest.raises(AssertionError):
            cp.partition_stripe(A, K, cp.GreedyBottleneckPartitioner(mdl, order=order), Pi, backend=hip)
    bad = Pi.asg.copy()
    bad[m // 2] = K + 1
    low = Pi.asg.copy()
    low[0] = 0
    for asg in (bad, low):
        for method in (cp.GreedyBottleneckPartitioner(mdl), cp.MagneticPartitioner()):
            with pytest.raises(AssertionError):
                cp.partition_stripe(A, K, method, cp.MapPartition(K, asg), backend=hip)
    with pytest.raises(AssertionError):                                       # Pi.K != K
        cp.partition_stripe(A, K, cp.GreedyBottleneckPartitioner(mdl), mm.row_partition("map", m, K + 1), backend=hip)
    with pytest.raises(AssertionError):                                       # Pi of another matrix's rows
        cp.partition_stripe(A, K, cp.GreedyBottleneckPartitioner(mdl), mm.row_partition("map", m - 1, K), backend=hip)
    neg = np.arange(n, dtype=np.int64)
    neg[n - 1] = -1
    with pytest.raises(AssertionError):
        cp.partition_stripe(A, K, cp.MagneticPartitioner(draws=neg), Pi, backend=hip)
    for method in (cp.MagneticPartitioner(), cp.GreedyBottleneckPartitioner(mdl)):
        with pytest.raises(NotImplementedError):
            cp.partition_stripe(A, K, method, backend=hip)
    for other in (cp.AffinePrimaryConnectivityModel(0, 10, 1, 0, 100), cp.AffineConnectivityModel(0, 10, 1, 100)):
        with pytest.raises(NotImplementedError):
            cp.partition_stripe(A, K, cp.GreedyBottleneckPartitioner(other), Pi, backend=hip)
    # the library's own refusal of another model kind, below the Python check
    asg = np.zeros(n, dtype=np.int64)
    rp, keep = cp.api._rowpart(Pi)
    rc, _, _ = hip.partition_greedy_bottleneck(A, K, cp.AffineConnectivityModel(0, 10, 1, 100).marshal(), rp, 0, None, asg)
    assert rc == 4
    # ... and the device is as it was: the same call with sound arguments
    got = cp.partition_stripe(A, K, cp.GreedyBottleneckPartitioner(mdl, seed=1), Pi, backend=hip)
    assert np.array_equal(got.asg, mm.greedy(A, K, Pi, mdl, draws.greedy_order(1, n))[0])
    # the reference's keywords are accepted and ignored
    again = cp.partition_stripe(A, K, cp.GreedyBottleneckPartitioner(mdl, seed=1), Pi, backend=hip, adj_A=object(), adj_net=object())
    assert again == got


@gpu
@pytest.mark.parametrize("which", ["magnetic", "greedy"])
def test_plaid_chain_equals_the_steps_by_hand(hip, which):
    """bin/test_table_bottleneck.jl:38-41: split_nets__map_local[__split_comm], split_nets__map_greedy[__split_comm]"""
    A = golden_matrices()["LPnetlib/lp_etamacro"]
    K = 4
    net = cp.AffineConnectivityModel(0, 10, 1, 100)
    comm = cp.AffinePrimaryConnectivityModel(0, 10, 1, 0, 100)
    loc = cp.AffineSecondaryConnectivityModel(0, 10, 1, 0, 100)
    second = cp.MagneticPartitioner(3) if which == "magnetic" else cp.GreedyBottleneckPartitioner(loc, seed=3)
    T = cp.adjointpattern(A, backend=hip)
    Phi0 = cp.partition_stripe(A, K, cp.BisectIndexBottleneckSplitter(net), backend=hip)
    Pi1 = cp.partition_stripe(T, K, second, Phi0, backend=hip)
    Phi2 = cp.partition_stripe(A, K, cp.BisectIndexBottleneckSplitter(comm), Pi1, backend=hip)
    assert isinstance(Pi1, cp.MapPartition) and Pi1.asg.shape == (A.m,) and isinstance(Phi2, cp.SplitPartition)
    for cls in (cp.AlternatingPartitioner, cp.AlternatingNetPartitioner):
        Pi, Phi = cp.partition_plaid(A, K, cls(cp.BisectIndexBottleneckSplitter(net), second), backend=hip)
        assert Pi == Pi1 and Phi == Phi0
        Pi, Phi = cp.partition_plaid(A, K, cls(cp.BisectIndexBottleneckSplitter(net), second, cp.BisectIndexBottleneckSplitter(comm)), backend=hip)
        assert Pi == Pi1 and Phi == Phi2
    # the map the second slot returned is what the model gives for the adjoint
    if which == "magnetic":
        assert np.array_equal(Pi1.asg, mm.magnetic(T, K, Phi0, draws.magnetic_draws(3, T.n)))
    else:
        assert np.array_equal(Pi1.asg, mm.greedy(T, K, Phi0, loc, draws.greedy_order(3, T.n), adj_A=A)[0])


@gpu
def test_permuting_partitioner_maps_back(hip):
    A = golden_matrices()["LPnetlib/lp_etamacro"]
    K = 6
    rcm = cp.CuthillMcKeePermuter()
    Pi = cp.MapPartition(K, np.arange(A.m) % K + 1)
    tau = cp.permute_stripe(A, rcm, backend=hip)
    B = cp.permute(A, None, tau, backend=hip)
    for inner in (cp.MagneticPartitioner(11), cp.GreedyBottleneckPartitioner(cp.AffineSecondaryConnectivityModel(0, 10, 1, 0, 100), seed=11)):
        got = cp.partition_stripe(A, K, cp.PermutingPartitioner(rcm, inner), Pi, backend=hip)
        inner_res = cp.partition_stripe(B, K, inner, Pi, backend=hip)
        assert isinstance(got, cp.MapPartition) and got == tau[inner_res]
        # told in A's columns: column tau.prm[j'] of A is column j' of B
        assert np.array_equal(got.asg[tau.prm - 1], inner_res.asg)
