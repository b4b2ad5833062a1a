"""Inputs of the pair-partition tests (tests/test_corank_model.py on the CPU, tests/test_pair_partition.py on the GPU) and
the reference they share: the co-ranks of every tile boundary from the key arrays alone, by numpy."""
import functools

import numpy as np

TILES = (64, 128, 6080)   # tile lengths: 64 x T records per coarse bracket, several brackets on a few 10^5 records
N = 150_000


def _subset(rng, keys, frac):
    return keys[rng.random(len(keys)) < frac]


def _stride(rng):
    s = (1 << 50) // (2 * N)
    u = np.arange(2 * N, dtype=np.uint64) * np.uint64(s) + rng.integers(0, s, 2 * N, dtype=np.uint64)
    return _subset(rng, u, 0.66), _subset(rng, u, 0.66), 25


def _even(rng):
    # even strides, no jitter: A and B on two grids of different pitch (ties where they meet)
    return np.arange(N, dtype=np.uint64) * np.uint64(3000), np.arange(2 * N, dtype=np.uint64) * np.uint64(1500), 25


def _iid(rng):
    u = np.unique(rng.integers(0, 1 << 50, 2 * N, dtype=np.uint64))
    return _subset(rng, u, 0.66), _subset(rng, u, 0.66), 25


def _stretches(rng):
    i = np.arange(2 * N, dtype=np.uint64)
    u = (i // np.uint64(3000) << np.uint64(40)) + (i % np.uint64(3000)) * np.uint64(4) + rng.integers(0, 4, 2 * N, dtype=np.uint64)
    return _subset(rng, u, 0.66), _subset(rng, u, 0.66), 32


def _a_below(rng):
    u = np.unique(rng.integers(0, 1 << 49, N, dtype=np.uint64))
    return u, u + np.uint64(1 << 49), 25


def _a_above(rng):
    a, b, k = _a_below(rng)
    return b, a, k


def _one_a(rng):
    b = np.unique(rng.integers(0, 1 << 50, 300_000, dtype=np.uint64))
    return b[len(b) // 3: len(b) // 3 + 1].copy(), b, 25


def _one_b(rng):
    a, b, k = _one_a(rng)
    return b, a + np.uint64(1), k


def _empty_a(rng):
    return np.zeros(0, dtype=np.uint64), np.unique(rng.integers(0, 1 << 50, N, dtype=np.uint64)), 25


def _empty_b(rng):
    a, b, k = _empty_a(rng)
    return b, a, k


def _identical(rng):
    u = np.unique(rng.integers(0, 1 << 50, N, dtype=np.uint64))
    return u, u.copy(), 25


def _half(rng):
    # A dense in the first half of the key range and absent in the second
    b = np.unique(rng.integers(0, 1 << 50, N, dtype=np.uint64))
    a = np.unique(rng.integers(0, 1 << 49, 2 * N, dtype=np.uint64))
    return a, b, 25


def _k32(rng):
    # the whole 64-bit range, keys 0 and 2^64 - 1 present: spans above 2^63 inside one bracket
    u = np.unique(np.concatenate([rng.integers(0, 1 << 64, 2 * N, dtype=np.uint64, endpoint=False), np.array([0, (1 << 64) - 1], dtype=np.uint64)]))
    a, b = _subset(rng, u, 0.5), _subset(rng, u, 0.5)
    a = np.unique(np.concatenate([a, u[:1]]))
    b = np.unique(np.concatenate([b, u[-1:]]))
    return a, b, 32


def _k32_ends(rng):
    # a bracket of few records that holds both ends of the key range, and equal end keys in both lists
    a = np.array([0, 1, (1 << 63), (1 << 64) - 1], dtype=np.uint64)
    b = np.array([0, (1 << 64) - 2, (1 << 64) - 1], dtype=np.uint64)
    return a, b, 32


def _consecutive(rng):
    # brackets whose keys are consecutive integers
    u = np.arange(2 * N, dtype=np.uint64) + np.uint64(1 << 30)
    return _subset(rng, u, 0.66), _subset(rng, u, 0.66), 25


INPUTS = {"stride": _stride, "even": _even, "iid": _iid, "stretches": _stretches, "a_below": _a_below, "a_above": _a_above, "one_a": _one_a,
          "one_b": _one_b, "empty_a": _empty_a, "empty_b": _empty_b, "identical": _identical, "half": _half, "k32": _k32, "k32_ends": _k32_ends,
          "consecutive": _consecutive}
GUIDABLE = ("stride", "even", "iid")   # where the guided search must need fewer probes than bisection (strictly, on the mean)


@functools.lru_cache(maxsize=None)
def keys(name):
    """(keys of A, keys of B, k): strictly ascending uint64 arrays"""
    rng = np.random.default_rng(sorted(INPUTS).index(name) + 100)
    a, b, k = INPUTS[name](rng)
    for x in (a, b):
        assert x.dtype == np.uint64 and (x[1:] > x[:-1]).all()
    return a, b, k


def boundaries(ka, kb, T):
    """uint64 [tiles + 1, 2]: the records of A and of B before every tile of T merged records, A first on ties, the B record
    of a pair that a diagonal cuts pulled into the earlier tile (as tile_nas of tests/test_pair_a_rows.py finds its a)"""
    rank_a = np.arange(len(ka)) + np.searchsorted(kb, ka, side="left")
    total = len(ka) + len(kb)
    diag = np.minimum(np.arange((total + T - 1) // T + 1) * T, total)
    a = np.searchsorted(rank_a, diag, side="left")
    b = diag - a
    can = (a > 0) & (b < len(kb))
    pair = np.zeros(len(a), dtype=bool)
    pair[can] = ka[a[can] - 1] == kb[b[can]]
    return np.stack([a, b + pair], axis=1).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def reference(name, T):
    ka, kb, _ = keys(name)
    return boundaries(ka, kb, T)
