"""gt4hip_pairwise_multi / gt4hip_table_pairwise through capi against tests/pairwise_model.py, number for number: every
lane-group width of the partial kernel (2 .. 32 lanes per row), one and several blocks of 32 list columns, both forms of the
count table (ragged: up to 32 lists in one launch of the N-way tile kernel; contiguous: by merges beyond 32 lists, or after
gt4hip_table_compact), and union sizes around a segment of the contiguous walk, a tile of the N-way tile kernel and a step of a
workgroup, all read from the sources (tests/pairwise_util.py)."""
import numpy as np
import pytest

import pairwise_model as PM
import pairwise_util as PU
import select_util as SU
from genometester4_amd import capi
from genometester4_amd.listio import make_records

pytestmark = pytest.mark.gpu

N_LISTS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32, 33, 64, 65, 100)
TOP = 0xffffffff


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


_sets = {}


def make_lists(n, size, k=25, seed=0, max_count=5, zero_counts=False):
    """n lists whose union has `size` words: word i lies in 1 + (i mod n) lists drawn at random, so rows that one list holds
    and rows that every list holds both occur once size >= n"""
    key = (n, size, k, seed, max_count, zero_counts)
    if key not in _sets:
        rng = np.random.default_rng(104729 * n + 31 * size + k + seed)
        universe = np.unique(rng.integers(0, 1 << (2 * k), size=size + size // 4 + 8, dtype=np.uint64, endpoint=False))
        universe = np.sort(rng.permutation(universe)[:size])
        assert len(universe) == size
        p = rng.permutation(1 + np.arange(size) % n)
        member = np.argsort(rng.random((n, size)), axis=0).argsort(axis=0) < p[None, :]
        lists = []
        for j in range(n):
            counts = rng.integers(0 if zero_counts else 1, max_count + 1, size=int(member[j].sum()), dtype=np.uint32)
            lists.append(make_records(universe[member[j]], counts))
        _sets[key] = (lists, PM.pairwise(lists))
    return _sets[key]


def check_forms(ctx, lists, want, k=25, ragged=None):
    """pairwise_multi, table_pairwise on the table as built and on the same table compacted"""
    n = len(lists)
    dev = [ctx.upload(l, k) for l in lists]
    shared, min_total = ctx.pairwise_multi(dev)
    assert shared.shape == min_total.shape == (n, n) and shared.dtype == min_total.dtype == np.uint64
    assert np.array_equal(shared, want[0]) and np.array_equal(min_total, want[1])
    assert ctx.last_pairwise_ms >= 0
    table = ctx.device_table(dev)
    if ragged is not None:
        assert bool(table.ragged) == ragged
    before = table.download()
    for form in ("as built", "compacted"):
        if form == "compacted":
            table.compact()
            assert not table.ragged
        shared, min_total = ctx.table_pairwise(table)
        assert np.array_equal(shared, want[0]) and np.array_equal(min_total, want[1]), (n, form)
    after = table.download()  # the table is only read
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    table.free()
    for l, d in zip(lists, dev):
        assert d.download().tobytes() == l.tobytes()
        d.free()


def union_sizes(n):
    """1, and one below, at and one above: a segment of the contiguous walk and a tile of the N-way tile kernel (a segment of a
    ragged table: a segment is one workgroup's share of the rows), and the rows a workgroup reads per step"""
    out = {1}
    for t in (SU.select_segment(), SU.nway_tile(), PU.pairwise_step(n)):
        out |= {t - 1, t, t + 1}
    return sorted(out)


def test_sizes_come_from_the_sources():
    assert SU.select_segment() == 4096 and PU.pairwise_block() == 32
    assert [PU.pairwise_step(n) for n in (1, 2, 3, 8, 9, 32, 33, 100)] == [512, 512, 256, 128, 64, 32, 32, 32]
    assert len(union_sizes(32)) >= 7 and len(union_sizes(3)) >= 7


@pytest.mark.parametrize("n", N_LISTS)
def test_every_number_of_lists_in_both_table_forms(ctx, n):
    size = SU.nway_tile() + 3 * PU.pairwise_step(n) + 17
    lists, want = make_lists(n, size)
    held = (PM.count_table(lists)[1] != 0).sum(axis=1)
    assert held.min() == 1 and held.max() == n  # rows that one list holds, rows that every list holds
    check_forms(ctx, lists, want, ragged=2 <= n <= 32)


@pytest.mark.parametrize("n", [3, 8, 32, 33, 65])
def test_union_sizes_around_segments_tiles_and_steps(ctx, n):
    for size in union_sizes(n):
        lists, want = make_lists(n, size)
        check_forms(ctx, lists, want)


@pytest.mark.parametrize("n", [2, 5, 33])
def test_a_count_of_zero_is_absence(ctx, n):
    lists, want = make_lists(n, 2 * PU.pairwise_step(n) + 77, seed=5, max_count=3, zero_counts=True)
    assert any(int((l["count"] == 0).sum()) for l in lists)
    assert all(int(want[0][j][j]) == int((lists[j]["count"] != 0).sum()) for j in range(n))
    check_forms(ctx, lists, want)


@pytest.mark.parametrize("n", [2, 9, 40])
def test_sums_of_counts_of_all_ones_pass_32_bits(ctx, n):
    lists = [l.copy() for l in make_lists(n, 600, seed=9)[0]]
    extra = make_records([3, 1 << 40, (1 << 50) - 1], [TOP, TOP, TOP])  # three rows of 0xffffffff in two lists
    for j in (0, n - 1):
        rest = lists[j][~np.isin(lists[j]["key"], extra["key"])]
        lists[j] = np.sort(np.concatenate([rest, extra]), order="key")
    want = PM.pairwise(lists)
    assert int(want[1][0][n - 1]) >= 3 * TOP > 1 << 32 and int(want[1][0][0]) > 1 << 32
    check_forms(ctx, lists, want)


@pytest.mark.parametrize("n", [2, 9, 33])
def test_an_empty_list_counts_towards_n_and_shares_nothing(ctx, n):
    lists = [l.copy() for l in make_lists(n, 1000)[0]]
    lists[n // 2] = lists[n // 2][:0]
    want = PM.pairwise(lists)
    assert not want[0][n // 2].any() and not want[0][:, n // 2].any() and not want[1][n // 2].any()
    check_forms(ctx, lists, want)
    empties = [l[:0] for l in lists]
    check_forms(ctx, empties, (np.zeros((n, n), dtype=np.uint64), np.zeros((n, n), dtype=np.uint64)))


@pytest.mark.parametrize("n", [3, 32, 40])
def test_identical_and_pairwise_disjoint_lists(ctx, n):
    one = make_lists(1, 2 * SU.nway_tile() + 5)[0][0]
    words, total = len(one), int(one["count"].astype(np.uint64).sum())
    same = PM.pairwise([one] * n)
    assert (same[0] == words).all() and (same[1] == total).all()
    check_forms(ctx, [one] * n, same)
    disjoint = [one[j::n] for j in range(n)]
    want = PM.pairwise(disjoint)
    assert np.array_equal(want[0], np.diag(np.diag(want[0]))) and int(np.trace(want[0])) == words
    check_forms(ctx, disjoint, want)


@pytest.mark.parametrize("k,size", [(1, 4), (5, 300), (16, 700), (32, 3000)])
def test_word_lengths(ctx, k, size):
    rng = np.random.default_rng(k)
    space = 1 << (2 * k)
    words = np.arange(space, dtype=np.uint64) if space <= 1024 else np.unique(rng.integers(0, space, size=size, dtype=np.uint64, endpoint=False))
    if k == 32:
        words[-1] = np.uint64(space - 1)  # the all-ones word
    lists = []
    for j in range(5):
        m = rng.random(len(words)) < 0.6
        lists.append(make_records(words[m], rng.integers(1, 9, size=int(m.sum()), dtype=np.uint32)))
    check_forms(ctx, lists, PM.pairwise(lists), k=k)


def test_the_goldens_of_the_reference(ctx):
    for case in PU.load_golden():
        check_forms(ctx, case["records"], PU.golden_matrices(case), k=case["word_length"])


def test_one_list_and_bad_arguments(ctx):
    lists = make_lists(3, 100)[0]
    one = lists[0]
    check_forms(ctx, [one], (np.array([[len(one)]], dtype=np.uint64), np.array([[int(one["count"].sum())]], dtype=np.uint64)))
    dev = [ctx.upload(l, 25) for l in lists[:2]] + [ctx.upload(lists[2], 24)]
    with pytest.raises(capi.Gt4HipError) as e:
        ctx.pairwise_multi(dev)
    assert e.value.code == capi.EWORDLEN
    for d in dev:
        d.free()
