"""The per-round kernel chain of the total-cost DP layer (csrc/dp_total.hip, csrc/dp_total_own.hip) against the path that never uses it.

The own-tile path of a round -- one launch for the two task scans and the round's verdict, tile map, block order that hands
its counters back as zeros, stream, and the two merges that sum a task's tile counts themselves -- is compared with the
flattened path (cp_set_option("dbg", 64): every long task stays in the flattened space; kernels of its own, scans of its own)
through cp_dp_layer with injected previous-layer rows that are not DP rows: cst and ptr must agree element for element, for
ConnectivityCosts and HyperedgeCut (second count), Int64 and integral Float64.
"""
import numpy as np
import pytest
import torch

from util import cp, suitesparse_shaped

pytestmark = pytest.mark.gpu

SCAN_TILE = 2048         # csrc/common.hpp: elements per block of the chained scans
LT = 256                 # csrc/dp_total.hpp: steps per tile

FIX_SERIAL = 16          # csrc/dp_total.hpp: tasks of up to FIX_SERIAL tiles are merged by one lane, longer ones by one block
MODELS = [cp.AffineConnectivityModel(1, 10, 1, 100), cp.AffineHyperedgeCutModel(0, 2, 1, 1, 3),
          cp.AffineConnectivityModel(0.0, 0.0, 0.0, 1.0), cp.AffineHyperedgeCutModel(0.0, 1.0, 0.0, -1.0, 2.0)]
IDS = ["conn-i64", "hyper-i64", "conn-f64", "hyper-f64"]


def w_rows(rng, n, dt, scale=1_000_000):
    """arbitrary, monotone and flat-with-wells previous layers (the wells at several densities: arg-min staircases whose steps
    -- the task lengths -- run from a few candidates to thousands of tiles)"""
    rows = [rng.integers(0, scale + 1, n + 1), np.sort(rng.integers(0, scale + 1, n + 1)), np.zeros(n + 1, dtype=np.int64)]
    for dens in (1e-2, 1.0 / 1024, 1.0 / 4096, 1.0 / 65536):
        rows.append(np.where(rng.random(n + 1) < dens, 0, scale * 8).astype(np.int64))
    return [r.astype(dt) for r in rows]


def run(hip, A, mdl, steps):
    """steps: (W, dbg, rows or None) per layer, on ONE DP handle (each layer is sized from the one before).  Returns (cst, ptr) per step."""
    n = A.n
    dev = torch.device("cuda", 0)
    dt = torch.int64 if mdl.dtype == cp.models.CP_I64 else torch.float64
    dp = hip.dp_begin(A, 3, 0, 0, mdl.marshal(), 1, n + 2)
    out = []
    try:
        for W, dbg, rows in steps:
            assert hip.set_option("dbg", dbg) == 0
            if rows is not None:
                hip.dp_set_rows(dp, rows[0], rows[1])
            prev = torch.from_numpy(np.ascontiguousarray(W)).to(dev)
            cur = torch.zeros(n + 1, dtype=dt, device=dev)
            hip.dp_layer(dp, 2, prev.data_ptr(), cur.data_ptr())
            out.append((cur.cpu().numpy(), hip.dp_ptr_row(dp, 2, n)))
    finally:
        hip.set_option("dbg", 0)
        hip.dp_destroy(dp)
    return out


def same(got, want, sl=slice(None)):
    for (c0, p0), (c1, p1) in zip(got, want):
        assert np.array_equal(p0[sl], p1[sl])
        assert np.array_equal(c0[sl], c1[sl])


@pytest.mark.parametrize("mi", range(len(MODELS)), ids=IDS)
def test_block_merge_carries_its_base_over_trips(hip, mi):
    """n = 2^21 + 3: the top rectangle's last row owns a task over its whole block, 2^20 columns = 4 096 tiles -- more than one
    2 048-tile trip of k_fix_own, so the base carried from trip to trip is used (asserted through the trip statistic)."""
    n = (1 << 21) + 3
    A = suitesparse_shaped(n, 3, 21)
    mdl = MODELS[mi]
    dt = np.int64 if mdl.dtype == cp.models.CP_I64 else np.float64
    Ws = w_rows(np.random.default_rng(40 + mi), n, dt)
    assert hip.set_option("stat_reset", 1) == 0
    got = run(hip, A, mdl, [(W, 0, None) for W in Ws])
    trips = hip.get_stat("fix_trips")
    want = run(hip, A, mdl, [(W, 64, None) for W in Ws])
    assert hip.get_stat("fix_trips") == trips                   # the reference path has no tiles of its own
    print("tasks merged in more than one trip:", trips)
    assert trips > 0
    same(got, want)


@pytest.mark.parametrize("mi", range(len(MODELS)), ids=IDS)
def test_both_sides_of_the_lane_block_split(hip, mi):
    """tasks of exactly 1, FIX_SERIAL (the longest a lane merges) and FIX_SERIAL + 1 tiles (the shortest a block merges)"""
    n = 300_007
    A = suitesparse_shaped(n, 4, 9)
    mdl = MODELS[mi]
    dt = np.int64 if mdl.dtype == cp.models.CP_I64 else np.float64
    Ws = w_rows(np.random.default_rng(50 + mi), n, dt)
    assert hip.set_option("stat_reset", 1) == 0
    got = run(hip, A, mdl, [(W, 0, None) for W in Ws])
    edges = hip.get_stat("fix_edges")
    want = run(hip, A, mdl, [(W, 64, None) for W in Ws])
    print("tile counts met (bit 0: 1, bit 1: %d, bit 2: %d): %d" % (FIX_SERIAL, FIX_SERIAL + 1, edges))
    assert edges == 7
    same(got, want)


@pytest.mark.parametrize("mi", range(len(MODELS)), ids=IDS)
def test_layers_around_a_forced_redo_and_a_row_tile(hip, mi):
    """a layer, a layer whose buffers are declared too small (dbg 2048: every round dropped by its verdict, the layer redone), a
    layer again, then a layer on a row tile: the layers after the redo and on the tile start from block counters that are zero
    (a dropped round counts no tiles, so the counters are clean by construction; the driver's extra clear is a safeguard)"""
    n = 70_001
    A = suitesparse_shaped(n, 5, 3)
    mdl = MODELS[mi]
    dt = np.int64 if mdl.dtype == cp.models.CP_I64 else np.float64
    Ws = w_rows(np.random.default_rng(60 + mi), n, dt)
    tile = (n // 3, n // 2 + 7)
    before = hip.get_stat("spec_redo")
    got = run(hip, A, mdl, [(Ws[0], 0, None), (Ws[3], 2048, None), (Ws[4], 0, None), (Ws[1], 0, None), (Ws[5], 0, tile)])
    assert hip.get_stat("spec_redo") > before                   # the second layer was redone
    want = run(hip, A, mdl, [(Ws[0], 64, None), (Ws[3], 64, None), (Ws[4], 64, None), (Ws[1], 64, None), (Ws[5], 64, tile)])
    same(got[:4], want[:4])
    same(got[4:], want[4:], slice(tile[0] - 1, tile[1] - 1))


# ---- the launch that ends a round's counting phase (k_round_scans through cp_test_round_scans) against numpy.cumsum
SCAN_N = [0, 1, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE, 1_000_000]


def excl(a):
    return np.concatenate([[0], np.cumsum(a.astype(np.int64))])


@pytest.mark.parametrize("nb", SCAN_N)
@pytest.mark.parametrize("na", SCAN_N)
def test_round_scans_against_cumsum(hip, na, nb):
    """both scans of the launch for every pair of counts (none, one, a block less one, whole blocks -- the last block then holds
    index n only --, a block and one, many blocks: look-back across blocks inside each range), the grid sized for more elements
    than the counts on the device say, three launches in a row on one workspace"""
    rng = np.random.default_rng(na * 7 + nb)
    a = rng.integers(0, 1000, na).astype(np.int32)
    b = rng.integers(0, 50, nb).astype(np.int32)
    for (ma, mb) in [(na + 1, nb + 1), (na + 3 * SCAN_TILE + 5, nb + SCAN_TILE)]:
        offs, toffs, res = hip.test_round_scans(a, ma, b, mb, reps=3)
        assert np.array_equal(offs, excl(a))
        assert np.array_equal(toffs, excl(b))
        T, NT = int(a.sum(dtype=np.int64)), int(b.sum(dtype=np.int64))
        assert res == {"T": T, "NT": NT, "nlong": na, "nown": nb, "ntile": -(-T // LT), "err": 0}


def test_round_scans_first_scan_alone(hip):
    """the flattened-only form (no own tiles): one scan, the verdict by its writer"""
    for na in SCAN_N:
        a = np.random.default_rng(na).integers(0, 1000, na).astype(np.int32)
        offs, _, res = hip.test_round_scans(a, na + SCAN_TILE + 1, np.zeros(0, np.int32), 1, two=False, reps=2)
        T = int(a.sum(dtype=np.int64))
        assert np.array_equal(offs, excl(a))
        assert res == {"T": T, "NT": 0, "nlong": na, "nown": 0, "ntile": -(-T // LT), "err": 0}


@pytest.mark.parametrize("na,nb", [(SCAN_TILE + 1, 1), (1, SCAN_TILE + 1), (1_000_000, 3 * SCAN_TILE), (3 * SCAN_TILE, 1_000_000), (5, 0), (0, 5)])
def test_round_scans_verdict_drops_the_round(hip, na, nb):
    """a total beyond its capacity, or a flag set earlier in the round: T, NT, nlong, nown read 0, err 1 -- whichever of the two
    scans finishes last (a long first scan with a short second one and the reverse)"""
    rng = np.random.default_rng(na + 3 * nb)
    a = rng.integers(1, 1000, na).astype(np.int32)
    b = rng.integers(1, 50, nb).astype(np.int32)
    T, NT = int(a.sum(dtype=np.int64)), int(b.sum(dtype=np.int64))
    dropped = {"T": 0, "NT": 0, "nlong": 0, "nown": 0, "ntile": 0, "err": 1}
    kept = {"T": T, "NT": NT, "nlong": na, "nown": nb, "ntile": -(-T // LT), "err": 0}
    ma, mb = na + 2 * SCAN_TILE, nb + 2 * SCAN_TILE
    assert hip.test_round_scans(a, ma, b, mb, cap_t=T, cap_nt=NT, reps=2)[2] == kept           # exactly at capacity
    if na:
        assert hip.test_round_scans(a, ma, b, mb, cap_t=T - 1, cap_nt=NT, reps=2)[2] == dropped
    if nb:
        assert hip.test_round_scans(a, ma, b, mb, cap_t=T, cap_nt=NT - 1, reps=2)[2] == dropped
    offs, toffs, res = hip.test_round_scans(a, ma, b, mb, err_in=1, reps=2)
    assert res == dropped
    assert np.array_equal(offs, excl(a)) and np.array_equal(toffs, excl(b))      # (the scans themselves are not undone)
