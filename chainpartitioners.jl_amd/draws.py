"""The draws of the map partitioners as a function: where the reference calls Julia's global RNG (rand(1:k),
rand(colptr[j]:colptr[j+1]-1), randperm(n); MagneticPartitioner.jl:10, :13, :72), this package takes the draws as arguments, and
without them uses

    draw(seed, stream, idx) = SplitMix64(key(seed, stream) + idx * 0x2545F4914F6CDD1D) >> 1

a counter hash of pure 64-bit integer arithmetic, shifted right by one bit so that it is a non-negative int64.  csrc/map_part.hip
states the same function for the device.  Stream 1: the draws of MagneticPartitioner; stream 2: the keys the visiting order of
GreedyBottleneckPartitioner is sorted by.  idx is the 1-based column."""
import numpy as np

_M64 = (1 << 64) - 1
_GOLDEN, _MIX1, _MIX2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
_STREAM, _INDEX = 0xD1342543DE82EF95, 0x2545F4914F6CDD1D
STREAM_MAGNETIC, STREAM_GREEDY = 1, 2


def _splitmix64(x):
    """SplitMix64 of a python int"""
    x = (x + _GOLDEN) & _M64
    z = ((x ^ (x >> 30)) * _MIX1) & _M64
    z = ((z ^ (z >> 27)) * _MIX2) & _M64
    return z ^ (z >> 31)


def stream_key(seed, stream):
    return _splitmix64((int(seed) + int(stream) * _STREAM) & _M64)


def draw(seed, stream, idx):
    """int64 array (or python int for a scalar idx) of the draws at the indices idx"""
    if np.isscalar(idx):
        return _splitmix64((stream_key(seed, stream) + int(idx) * _INDEX) & _M64) >> 1
    idx = np.asarray(idx).astype(np.uint64)
    with np.errstate(over="ignore"):
        x = np.uint64(stream_key(seed, stream)) + idx * np.uint64(_INDEX) + np.uint64(_GOLDEN)
        z = (x ^ (x >> np.uint64(30))) * np.uint64(_MIX1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(_MIX2)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(1)).astype(np.int64)


def magnetic_draws(seed, n):
    """u_j of MagneticPartitioner(seed) for the columns 1 .. n"""
    return draw(seed, STREAM_MAGNETIC, np.arange(1, n + 1, dtype=np.int64))


def greedy_order(seed, n):
    """the visiting order of GreedyBottleneckPartitioner(mdl, seed): the columns 1 .. n ascending by (draw(seed, 2, j), j)"""
    return np.argsort(draw(seed, STREAM_GREEDY, np.arange(1, n + 1, dtype=np.int64)), kind="stable").astype(np.int64) + 1
