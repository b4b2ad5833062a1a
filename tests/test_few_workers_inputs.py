"""The inputs of tests/test_few_workers_gpu.py, built and checked without a GPU: what that file's cases rely on is asserted
here on the lists themselves and on the CPU oracle's results -- keys below and above the high cutoff, ADD sums that wrap to 0
and to 1, NUMBER's all-kept and all-dropped cutoffs, the clustered and the uniform stretch of the mixed input, narrow and wide
stretches, two sample levels with a long level-1 launch, the tables' rows per tile on both sides of one batch of the LDS
row area, and the exact tile counts of the scanner and short-loop cases."""
import pytest

import test_few_workers_gpu as F


@pytest.mark.parametrize("inst", list(F.INSTANCES))
def test_rule_inputs(inst):
    lists = F._wrap_input(inst)  # (asserts the wraps)
    for rule in (F.ADD, F.MAX):
        assert F.high_cutoff(lists, rule) >= 3
    assert F.number_cutoffs(lists, 3) == (2, 4)


def test_tile_path_inputs():
    F.mixed_lists()
    F.narrow_and_wide_lists()
    for path in ("vt99", "disjoint", "cut8", "cut12"):
        lists = F._path_case(path)[0]
        assert 300_000 <= sum(len(x) for x in lists) <= 1_100_000
    for x in F.disjoint_lists():  # no two lists share a key range
        assert int(x["key"][0]) >> 30 == int(x["key"][-1]) >> 30


@pytest.mark.parametrize("inst,universe,g", F.LEVEL_CASES)
def test_sample_level_inputs(inst, universe, g):
    F.sample_level_lists(inst, universe, g)


@pytest.mark.parametrize("n_lists,name", F.TABLE_CASES, ids=["%d-%s" % c for c in F.TABLE_CASES])
def test_table_inputs(n_lists, name):
    lists = F._table_input(name, n_lists)
    width = 8 if n_lists <= 8 else 32
    tiles = F.level_tiles([len(x) for x in lists], width, F.auto_g(n_lists, width))
    assert tiles >= F.MIN_PER_WORKER * max(F.OTHER_GRIDS)
    if name == "skewed" and n_lists >= 8:  # more than one batch of rows in some tile, of the union and of list 0
        assert F.rows_need_batches(lists, tiles, False) and F.rows_need_batches(lists, tiles, True)
    if name == "same":                     # one batch in every tile
        assert all(len(x) == len(lists[0]) for x in lists) and F.TILE // n_lists <= F.ROWW // n_lists


def test_exact_tile_counts():
    for tiles in (63, 64, 65, 8 * 64 + 10):
        assert F.level_tiles([F.SAMPLE[8] * (tiles - 2) + 5] * 4, 8, F.SCAN_G) == tiles
    assert F.level_tiles([700, 800, 900, 1000], 8, F.SCAN_G) == 1
    assert F.level_tiles((1300, 1300, 1100), 8, F.auto_g(3, 8)) == 1
    for tiles, g in F.SHORT_G.items():
        assert F.level_tiles(F.SHORT_SIZES, 8, g) == tiles
    for ops in (1, 15):
        tile = F.V.merge_tile_records(1, ops)
        for tiles in range(1, 6):
            n = (tiles * tile - 100) // 2
            assert F.V.compare_launches(ops, 0, F.C_EDGE, 0, n, n + 1).tiles == tiles
