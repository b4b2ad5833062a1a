"""The pair partition on the GPU (k_partition_coarse, k_partition: gt4hip_kernels.hip on gt4hip_corank.h) and the workspace
zeroing folded into its launch.

gt4hip_pair_partition runs the partition launch alone with any tile length, so lists of a few 10^5 records are cut into
thousands of tiles over many coarse brackets: the tile ranges it returns are held against numpy's co-ranks
(tests/partition_inputs.py) for every input, tile lengths 64, 128 and 6080, with option "part_guided" 0 (guided) and -1
(bisection).  Then -i, -u and -d -c 2 run on three of the inputs against the CPU oracle -- records and totals -- on the
single-pass path, the two-pass path and count-only, with both option values: the merge launch finds its control block
and its descriptor words zeroed by the partition launch alone.  Two calls in a row on one context, the second one
smaller and laid out differently in the same workspace, would show stale descriptor words."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle_lib as O  # noqa: E402
import partition_inputs as P  # noqa: E402
from genometester4_amd.listio import make_records  # noqa: E402

MERGED = ("iid", "identical", "k32")   # the inputs of the merge calls
CALLS = ((2, 1), (1, 1), (4, 2))       # (ops, cutoff): -i, -u, -d -c 2
PATHS = (("single_pass", {}, False), ("two_pass", {"two_pass": 1}, False), ("count_only", {}, True))


@functools.lru_cache(maxsize=None)
def records(name):
    ka, kb, k = P.keys(name)
    rng = np.random.default_rng(7)
    return make_records(ka, rng.integers(1, 5, len(ka), dtype=np.uint32)), make_records(kb, rng.integers(1, 5, len(kb), dtype=np.uint32)), k


@functools.lru_cache(maxsize=None)
def oracle(name, ops, cutoff, head=None):
    A, B, _ = records(name)
    if head:
        A, B = A[:head], B[:head]
    return O.compare(A, B, ops, 0, cutoff)


@pytest.fixture(scope="module")
def ctx():
    from genometester4_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def dev(ctx):
    made = {}

    def get(name, head=None):
        if (name, head) not in made:
            A, B, k = records(name)
            made[(name, head)] = (ctx.upload(A[:head] if head else A, k), ctx.upload(B[:head] if head else B, k))
        return made[(name, head)]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("guided", (0, -1))
@pytest.mark.parametrize("name", sorted(P.INPUTS))
def test_tile_ranges(ctx, dev, name, guided):
    a, b = dev(name)
    try:
        ctx.set_option("part_guided", guided)
        for T in P.TILES:
            got = ctx.pair_partition(a, b, T)
            ref = P.reference(name, T)
            assert got.shape == ref.shape, (name, T, got.shape, ref.shape)
            bad = np.flatnonzero((got != ref).any(axis=1))
            assert not len(bad), (name, T, guided, bad[:5], got[bad[:5]], ref[bad[:5]])
    finally:
        ctx.set_option("part_guided", 0)


def check(ctx, a, b, exp, ops, cutoff, count_only, what):
    st, out, _ = ctx.compare(a, b, ops, 0, cutoff, 0, 1, count_only)
    for bit in (1, 2, 4, 8):
        if not ops & bit:
            continue
        n_o, t_o, r_o = exp[bit]
        assert st[bit] == (n_o, t_o), (what, bit, st[bit], (n_o, t_o))
        if not count_only:
            got = out[bit].download()
            out[bit].free()
            assert got.tobytes() == r_o.tobytes(), (what, bit)


@pytest.mark.gpu
@pytest.mark.parametrize("guided", (0, -1))
@pytest.mark.parametrize("path", PATHS, ids=[p[0] for p in PATHS])
@pytest.mark.parametrize("name", MERGED)
def test_merges_on_the_folded_zeroing(ctx, dev, name, path, guided):
    _, opts, count_only = path
    a, b = dev(name)
    try:
        ctx.set_option("part_guided", guided)
        for o, v in opts.items():
            ctx.set_option(o, v)
        for ops, cutoff in CALLS:
            check(ctx, a, b, oracle(name, ops, cutoff), ops, cutoff, count_only, (name, path[0], guided, ops, cutoff))
        assert ctx.get_counter("single_pass_fallbacks") == 0
    finally:
        ctx.set_option("part_guided", 0)
        ctx.set_option("two_pass", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("guided", (0, -1))
def test_smaller_call_after_a_larger_one(ctx, dev, guided):
    """all four streams of ~4 x 10^5 records (two rows of 64 tiles: every stream's agg words are written), then the first 5000
    records of each list in the same workspace: one row, whose carries lie where the larger call's agg words lay"""
    a, b = dev("iid")
    sa, sb = dev("iid", 5000)
    try:
        ctx.set_option("part_guided", guided)
        for ops, cutoff in ((15, 2), (2, 1)):
            check(ctx, a, b, oracle("iid", 15, 2), 15, 2, False, ("large", guided))
            check(ctx, sa, sb, oracle("iid", ops, cutoff, 5000), ops, cutoff, False, ("small", guided, ops))
        assert ctx.get_counter("single_pass_fallbacks") == 0
        assert ctx.get_counter("partition_us") > 0
    finally:
        ctx.set_option("part_guided", 0)
