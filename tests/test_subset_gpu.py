"""gt4hip_list_subset through capi against the serial walk of tests/subset_model.py (the reference's loop restated), at
the sizes where the tiling can go wrong: around a wavefront, around a tile ("subset_tile" items), several tiles, and
enough items and records for the scans to take more than one level; for rand, records whose occurrences straddle a
tile boundary or cover several tiles.  Output records, n_words, total_count, "subset_passes", the input left as it was;
and the jump-ahead table against stepping the model's affine powers (host code)."""
import numpy as np
import pytest

import subset_model as SM
from genometester4_amd import capi
from genometester4_amd.listio import make_records

K = 25
_walks = {}


def _want(key, rec, method, size, x0):
    """the serial walk of a case, computed once"""
    if key not in _walks:
        try:
            _walks[key] = SM.serial_walk(rec, method, size, x0)
        except SM.Shortfall as e:
            _walks[key] = e
    return _walks[key]


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tile(ctx):
    t = ctx.get_counter("subset_tile")
    assert t >= 64 and t % 64 == 0
    return t


def _check(ctx, rec, method, size, seed):
    x0 = SM.state48(seed)
    items = SM.Items(rec, method).items
    want = _want((rec.tobytes(), method, size, x0), rec, method, size, x0)
    lst = ctx.upload(rec, K)
    if isinstance(want, SM.Shortfall):
        with pytest.raises(capi.Gt4HipError) as e:
            ctx.subset(lst, method, size, x0)
        assert e.value.code == capi.EINVAL
        assert SM.METHOD_NAMES[method] + " %d" % size in str(e.value) and "only %d of %d" % (want.reached, size) in str(e.value)
    else:
        n_words, total, out = ctx.subset(lst, method, size, x0)
        got = out.download()
        assert got.tobytes() == want.tobytes(), (method, len(rec), size)
        assert (n_words, total) == (len(want), int(want["count"].astype(np.uint64).sum()))
        passes = ctx.get_counter("subset_passes")
        assert 1 <= passes <= items + 1, passes
        out.free()
    assert lst.download().tobytes() == rec.tobytes()  # the input is only read
    lst.free()


def _sizes(items):
    return sorted({1, items // 2, items} - {0})


def _edge_items(tile):
    return [1, 2, 63, 64, 65, tile - 1, tile, tile + 1, 3 * tile + 5]


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(9))
def test_unique_methods_at_the_tile_edges(ctx, tile, which):
    n = _edge_items(tile)[which]
    rec = SM.make_list(100 + which, n, K, 30)
    for size in _sizes(n):
        _check(ctx, rec, SM.RAND_UNIQUE, size, 7)
    # rand_weighted_unique falls short at large sizes: the error is part of the check
    for size in sorted({1, max(1, n // 5), n // 2, n} - {0}):
        _check(ctx, rec, SM.RAND_WEIGHTED_UNIQUE, size, 7)


def _counts_with_sum(rng, n, total):
    """n counts >= 1 that add up to `total`"""
    cuts = np.sort(rng.choice(np.arange(1, total), size=n - 1, replace=False)) if n > 1 else np.zeros(0, dtype=np.int64)
    return np.diff(np.concatenate([[0], cuts, [total]])).astype(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(9))
def test_rand_at_the_tile_edges(ctx, tile, which):
    items = _edge_items(tile)[which]
    rng = np.random.default_rng(200 + which)
    n = min(items, 1 + items // 3)
    rec = SM.make_list(200 + which, n, K, 1)
    rec["count"] = _counts_with_sum(rng, n, items)
    for size in _sizes(items):
        _check(ctx, rec, SM.RAND, size, 11)


@pytest.mark.gpu
def test_rand_records_that_straddle_and_cover_tiles(ctx, tile):
    # record 1 straddles the first tile boundary, record 3 covers tiles 2 .. 4 whole, record 4 has no occurrence
    counts = np.array([tile - 3, 7, tile - 4, 3 * tile, 0, 5, 2 * tile + 1, 1], dtype=np.uint32)
    rec = make_records(SM.make_list(300, len(counts), K, 1)["key"], counts)
    items = int(counts.sum())
    for size in (1, 9, items // 2, items - 1, items, items + 1):
        _check(ctx, rec, SM.RAND, size, 13)


@pytest.mark.gpu
def test_seventy_thousand_items(ctx, tile):
    """more than one level in the scan over the records (and over the tiles, should a tile ever be small)"""
    n = 70_001
    rec = SM.make_list(400, n, K, 1)
    _check(ctx, rec, SM.RAND_UNIQUE, n // 2, 3)
    _check(ctx, rec, SM.RAND_WEIGHTED_UNIQUE, n // 4, 3)  # counts all 1: the walk is rand_unique's and ends
    rec = SM.make_list(401, 23_000, K, 5)
    _check(ctx, rec, SM.RAND, int(rec["count"].sum()) // 2, 3)
    _check(ctx, rec, SM.RAND_WEIGHTED_UNIQUE, 2_000, 3)


@pytest.mark.gpu
def test_more_tiles_than_one_scan_tile_holds(ctx, tile):
    """thousands of tiles, so that the scan over the tile sums has two levels.  A serial walk of so many items takes the
    model minutes, so SIZE is all of them: out == in at every item, every ratio is 1, every draw is below it, and the
    list comes back as it is (less the record without occurrences); every carry-in is the number of items before it."""
    rec = SM.make_list(500, 3_000, K, 6_000)
    rec["count"][1234] = 0
    items = int(rec["count"].astype(np.uint64).sum())
    assert items // tile > 2048
    lst = ctx.upload(rec, K)
    n_words, total, out = ctx.subset(lst, SM.RAND, items, SM.state48(17))
    assert out.download().tobytes() == rec[rec["count"] > 0].tobytes()
    assert (n_words, total) == (len(rec) - 1, items)
    assert 1 <= ctx.get_counter("subset_passes") <= items + 1
    # a third of them: what can be said without the walk
    n_words, total, out = ctx.subset(lst, SM.RAND, items // 3, SM.state48(17))
    got = out.download()
    at = np.searchsorted(rec["key"], got["key"])
    assert (n_words, total) == (len(got), items // 3) and int(got["count"].astype(np.uint64).sum()) == items // 3
    assert np.array_equal(rec["key"][at], got["key"]) and np.all(got["count"] <= rec["count"][at]) and np.all(got["count"] > 0)


@pytest.mark.gpu
def test_empty_cases_and_bad_arguments(ctx):
    rec = SM.make_list(600, 100, K, 3)
    lst = ctx.upload(rec, K)
    for method in (SM.RAND, SM.RAND_UNIQUE, SM.RAND_WEIGHTED_UNIQUE):
        n_words, total, out = ctx.subset(lst, method, 0, SM.state48(1))
        assert (n_words, total, out.n_words) == (0, 0, 0)
        assert ctx.get_counter("subset_passes") == 0
        empty = ctx.upload(rec[:0], K)
        n_words, total, out = ctx.subset(empty, method, 5, SM.state48(1))
        assert (n_words, total, out.n_words) == (0, 0, 0)
    for method, size in ((SM.RAND_UNIQUE, 101), (SM.RAND, int(rec["count"].sum()) + 1)):
        with pytest.raises(capi.Gt4HipError) as e:
            ctx.subset(lst, method, size, SM.state48(1))
        assert e.value.code == capi.EINVAL and "only" in str(e.value)
    with pytest.raises(capi.Gt4HipError) as e:
        ctx.subset(lst, 3, 1, SM.state48(1))
    assert e.value.code == capi.EINVAL


def test_jump_ahead_table_against_the_models_affine_powers():
    """host code: no device"""
    powers = SM.affine_powers()
    for x0 in (SM.state48(0), SM.state48(7), SM.state48(-2)):
        # 2^40 steps: one entry of the table; 2^32 + 3: one entry, then three single steps
        a, c = powers[40]
        assert capi.subset_state_at(x0, 1 << 40) == (a * x0 + c) & SM.LCG_MASK
        a, c = powers[32]
        x = (a * x0 + c) & SM.LCG_MASK
        for _ in range(3):
            x = (SM.LCG_A * x + SM.LCG_C) & SM.LCG_MASK
        assert capi.subset_state_at(x0, (1 << 32) + 3) == x
        for k in range(48):
            a, c = powers[k]
            assert capi.subset_state_at(x0, 1 << k) == (a * x0 + c) & SM.LCG_MASK
        x = x0
        for pos in range(70):
            assert capi.subset_state_at(x0, pos) == x
            x = (SM.LCG_A * x + SM.LCG_C) & SM.LCG_MASK
        assert capi.subset_state_at(x0, 1 << 48) == x0
