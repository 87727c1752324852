"""pack_plaid (AlternatingPacker.jl:18-32, :40-53) is host orchestration over adjointpattern and pack_stripe: on the CPU oracle
backend it must equal the hand-written sequence of pack_stripe calls on A and its adjoint; the greedy chunkers, which only the HIP
backend has, refuse the oracle backend by name."""
import numpy as np
import pytest

from util import cp, sprand, golden_matrices


def block_chunker(w):
    mdl = cp.BlockComponentCostModel(0, 0, (2, lambda x: x), (2, lambda x: 2 * x))
    return cp.DynamicTotalChunker(cp.ConstrainedCost(mdl, cp.VertexCount(), w))


def conn_chunker(w):
    return cp.DynamicTotalChunker(cp.ConstrainedCost(cp.AffineConnectivityModel(0, 3, 1, 3), cp.VertexCount(), w))


def mats():
    rng = np.random.default_rng(3)
    g = golden_matrices()
    return [sprand(9, 14, 0.3, rng), sprand(20, 20, 0.15, rng), g["LPnetlib/lpi_itest6"], g["Pajek/GD99_c"]]


def method_lists():
    return [[cp.EquiChunker(2), block_chunker(4)],
            [cp.EquiChunker(2), block_chunker(4), block_chunker(3)],
            [cp.EquiChunker(3), block_chunker(4), block_chunker(4), block_chunker(2)]]


def test_alternating_packer_is_the_sequence_of_pack_stripe_calls(orc):
    for A in mats():
        T = cp.adjointpattern(A, backend=orc)
        for mtds in method_lists():
            Pi, Phi = cp.pack_plaid(A, cp.AlternatingPacker(*mtds), backend=orc)
            phi = cp.pack_stripe(A, mtds[0], backend=orc)
            pi = cp.pack_stripe(T, mtds[1], phi, backend=orc)
            for i, mtd in enumerate(mtds[2:], start=1):
                if i % 2 == 1:
                    phi = cp.pack_stripe(A, mtd, pi, backend=orc)
                else:
                    pi = cp.pack_stripe(T, mtd, phi, backend=orc)
            assert Pi == pi and Phi == phi, (A, len(mtds))
            assert Phi.spl[-1] == A.n + 1 and Pi.spl[-1] == A.m + 1
            # the adjoint handed in is the adjoint computed
            assert cp.pack_plaid(A, cp.AlternatingPacker(*mtds), adj_A=T, backend=orc) == (Pi, Phi)


def test_symmetric_packer_is_the_sequence_of_pack_stripe_calls(orc):
    for A in mats():
        if A.m != A.n:
            continue
        T = cp.adjointpattern(A, backend=orc)
        for mtds in ([cp.EquiChunker(2)], [cp.EquiChunker(2), block_chunker(4)], [cp.EquiChunker(3), block_chunker(4), conn_chunker(3)],
                     [cp.EquiChunker(2), block_chunker(4), block_chunker(3), block_chunker(4)]):
            Pi, Phi = cp.pack_plaid(A, cp.SymmetricPacker(*mtds), backend=orc)
            pi = cp.pack_stripe(A, mtds[0], backend=orc)
            for i, mtd in enumerate(mtds[1:], start=1):
                pi = cp.pack_stripe(A if i % 2 == 1 else T, mtd, pi, backend=orc)
            assert Pi == pi and Phi == pi, (A, len(mtds))


def test_greedy_chunkers_name_the_backend_that_lacks_them(orc):
    A = sprand(6, 9, 0.4, np.random.default_rng(1))
    for meth in (cp.StrictChunker(8), cp.OverlapChunker(0.9, 8)):
        with pytest.raises(NotImplementedError, match="oracle"):
            cp.pack_stripe(A, meth, backend=orc)
        with pytest.raises(NotImplementedError, match="oracle"):
            cp.pack_plaid(A, cp.AlternatingPacker(meth, meth), backend=orc)


def test_unknown_methods_keep_their_message(orc):
    class Other:
        pass
    A = sprand(6, 9, 0.4, np.random.default_rng(1))
    with pytest.raises(NotImplementedError, match="method Other is outside the hot path"):
        cp.pack_stripe(A, Other(), backend=orc)
    with pytest.raises(NotImplementedError, match="pack_plaid: method Other is outside the hot path"):
        cp.pack_plaid(A, Other(), backend=orc)
