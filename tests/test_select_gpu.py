"""gt4hip_select_multi / gt4hip_table_select through capi against tests/select_model.py, byte for byte: every lane-group
width of the decision kernel (2 .. 64 lanes per row, and rows longer than 64 columns), both forms of the count table (ragged:
up to 32 lists in one launch of the N-way tile kernel; contiguous: by merges beyond 32 lists, or after gt4hip_table_compact),
and union sizes around the tiles of the kernels involved, all read from the sources (tests/select_util.py)."""
import numpy as np
import pytest

import oracle_lib as O
import select_model as SM
import select_util as SU
from genometester4_amd import capi
from genometester4_amd.listio import make_records

pytestmark = pytest.mark.gpu

N_LISTS = (2, 3, 8, 9, 32, 33, 70)
ADD, MAX, NUMBER = capi.RULE_ADD, capi.RULE_MAX, capi.RULE_NUMBER


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def union_sizes():
    """0, 1, and around one and beyond three tiles of the select emit kernel, of a segment of a contiguous table and of the
    N-way tile kernel (whose tiles are the segments of a ragged table)"""
    out = {0, 1}
    for t in (SU.select_tile(), SU.select_segment(), SU.nway_tile()):
        out |= {t - 1, t, t + 1, 3 * t + 17}
    return sorted(out)


def test_tile_sizes_come_from_the_sources():
    assert SU.select_tile() >= 256 and SU.select_segment() % SU.select_tile() == 0 and SU.nway_tile() >= 1024
    assert len(union_sizes()) >= 8


_sets = {}


def make_lists(n, size, k=25, seed=0, max_count=5, zero_counts=False):
    """n lists whose union has `size` words of a shared universe: word i lies in 1 + (i mod n) lists drawn at random, so
    every p from 1 to n occurs once size >= n.  k = 32: the all-ones word is one of them."""
    key = (n, size, k, seed, max_count, zero_counts)
    if key not in _sets:
        rng = np.random.default_rng(7919 * n + 31 * size + k + seed)
        space = 1 << (2 * k)
        if space <= 1 << 20:
            assert size <= space
            universe = np.sort(rng.permutation(space)[:size]).astype(np.uint64)
        else:
            universe = np.unique(rng.integers(0, space, size=size + size // 4 + 8, dtype=np.uint64, endpoint=False))
            universe = np.sort(rng.permutation(universe)[:size])
        if size and k in (5, 32):
            universe[-1] = np.uint64(space - 1)  # the all-ones word (already the largest, or larger than all)
            universe = np.unique(universe)
        assert len(universe) == size
        p = rng.permutation(1 + np.arange(size) % n)
        member = np.argsort(rng.random((n, size)), axis=0).argsort(axis=0) < p[None, :]
        lists = []
        for j in range(n):
            counts = rng.integers(0 if zero_counts else 1, max_count + 1, size=int(member[j].sum()), dtype=np.uint32)
            lists.append(make_records(universe[member[j]], counts))
        _sets[key] = lists
    return _sets[key]


_models = {}


def model(tag, lists, m, x, cutoff, rule, ovr):
    """the model's answer, computed once per case"""
    key = (tag, m, x, cutoff, rule, ovr)
    if key not in _models:
        _models[key] = SM.select(lists, m, x, cutoff, rule, ovr)
    return _models[key]


def pairs(n, every=False):
    if every:
        return [(m, x) for m in range(1, n + 1) for x in range(m, n + 1)]
    out = {(1, n), (n, n), (1, 1), (1, n - 1) if n > 1 else (1, 1), (2, n)}
    if n >= 4:
        out |= {(2, n - 1), (n // 2, n // 2 + 1)}
    return sorted(out)


def check(ctx, tag, lists, k, m, x, cutoff=1, rule=0, ovr=1, dev=None):
    rc_w, n_w, t_w, rec_w = model(tag, lists, m, x, cutoff, rule, ovr)
    assert rc_w == 0
    own = dev is None
    if own:
        dev = [ctx.upload(l, k) for l in lists]
    rc, n, t, out = ctx.select_multi(dev, m, x, cutoff, rule, ovr)
    got = out.download()
    assert (rc, n, t) == (0, n_w, t_w), (tag, m, x, cutoff, rule)
    assert got.tobytes() == rec_w.tobytes(), (tag, m, x, cutoff, rule)
    assert out.word_length == k
    out.free()
    if own:
        for d in dev:
            d.free()


@pytest.mark.parametrize("n", N_LISTS)
def test_union_sizes_around_the_tiles(ctx, n):
    for size in union_sizes():
        lists = make_lists(n, size)
        assert size < n or sorted(set(SM.presence(lists)[1].tolist())) == list(range(1, n + 1))
        dev = [ctx.upload(l, 25) for l in lists]
        for m, x in pairs(n):
            check(ctx, ("sizes", n, size), lists, 25, m, x, dev=dev)
        for d in dev:
            d.free()


@pytest.mark.parametrize("n", [x for x in N_LISTS if x <= 8])
def test_every_band_of_up_to_eight_lists(ctx, n):
    size = 3 * SU.select_tile() + 17
    lists = make_lists(n, size)
    dev = [ctx.upload(l, 25) for l in lists]
    for m, x in pairs(n, every=True):
        check(ctx, ("sizes", n, size), lists, 25, m, x, dev=dev)
    for d in dev:
        d.free()


@pytest.mark.parametrize("n", N_LISTS)
@pytest.mark.parametrize("rule,ovr", [(ADD, 1), (MAX, 1), (NUMBER, 3), (NUMBER, 2), (0, 1)], ids=["add", "max", "number3", "number2", "default"])
def test_rules_and_cutoffs(ctx, n, rule, ovr):
    size = SU.nway_tile() + 1
    lists = make_lists(n, size, max_count=4)
    dev = [ctx.upload(l, 25) for l in lists]
    above = 4 * n + 1  # above every count, folded or not
    for cutoff in (1, 3, above):
        for m, x in [(1, n), (n, n), (2, n - 1) if n > 2 else (1, 1)]:
            check(ctx, ("rules", n), lists, 25, m, x, cutoff, rule, ovr, dev=dev)
    rc, cnt, tot, rec = model(("rules", n), lists, 1, n, above, rule, ovr)
    assert cnt == 0 and len(rec) == 0
    for d in dev:
        d.free()


@pytest.mark.parametrize("n", [2, 9, 33])
def test_an_empty_list_counts_towards_n_and_holds_nothing(ctx, n):
    size = SU.select_tile() + 1
    lists = [l.copy() for l in make_lists(n, size)]
    lists[n // 2] = lists[n // 2][:0]
    for m, x in pairs(n):
        check(ctx, ("empty", n), lists, 25, m, x)
    assert model(("empty", n), lists, n, n, 1, 0, 1)[1] == 0  # no word is in every list
    empties = [l[:0] for l in lists]
    for m, x in [(1, n), (n, n)]:
        check(ctx, ("all_empty", n), empties, 25, m, x)
    check(ctx, ("one_nonempty", n), empties[:-1] + [make_lists(n, size)[0]], 25, 1, 1)


@pytest.mark.parametrize("n", [3, 8, 32, 40])
def test_identical_and_pairwise_disjoint_lists(ctx, n):
    one = make_lists(1, 2 * SU.select_tile() + 5)[0]
    same = [one] * n
    for m, x in [(1, n), (n, n), (1, n - 1), (n - 1, n)]:
        check(ctx, ("same", n), same, 25, m, x)
        check(ctx, ("same", n), same, 25, m, x, 1, MAX)
    assert model(("same", n), same, n, n, 1, 0, 1)[1] == len(one) and model(("same", n), same, 1, n - 1, 1, 0, 1)[1] == 0
    disjoint = [one[j::n] for j in range(n)]
    for m, x in [(1, n), (1, 1), (2, n), (n, n)]:
        check(ctx, ("disjoint", n), disjoint, 25, m, x)
    assert model(("disjoint", n), disjoint, 1, 1, 1, 0, 1)[1] == len(one) and model(("disjoint", n), disjoint, 2, n, 1, 0, 1)[1] == 0


@pytest.mark.parametrize("n", [2, 5, 33])
def test_a_count_of_zero_does_not_hold_a_word(ctx, n):
    lists = make_lists(n, SU.select_tile() + 77, seed=5, max_count=3, zero_counts=True)
    assert any(int((l["count"] == 0).sum()) for l in lists)
    for rule, ovr in [(ADD, 1), (MAX, 1), (NUMBER, 2)]:
        for cutoff in (0, 1, 2):
            for m, x in [(1, n), (n, n), (1, 1), (2, n)]:
                check(ctx, ("zeros", n), lists, 25, m, x, cutoff, rule, ovr)


@pytest.mark.parametrize("k,size", [(5, 1024), (5, 300), (25, 3000), (32, 3000), (32, 1), (1, 4)])
def test_word_lengths_and_the_all_ones_word(ctx, k, size):
    for n in (3, 9):
        lists = make_lists(n, size, k=k)
        if k in (5, 32):
            assert max(int(l["key"].max()) for l in lists if len(l)) == (1 << (2 * k)) - 1
        for m, x in pairs(n):
            check(ctx, ("k", k, size, n), lists, k, m, x)


@pytest.mark.parametrize("n", [3, 33])
def test_count_only_and_a_list_the_caller_brings(ctx, n):
    lists = make_lists(n, 3 * SU.select_tile() + 17)
    dev = [ctx.upload(l, 25) for l in lists]
    for m, x in [(1, n), (2, n - 1), (n, n)]:
        rc_w, n_w, t_w, rec_w = model(("sizes", n, 3 * SU.select_tile() + 17), lists, m, x, 1, 0, 1)
        assert ctx.select_multi(dev, m, x, count_only=True) == (0, n_w, t_w, None)
        mine = ctx.alloc(max(n_w, 1) + 3, 25)
        rc, cnt, tot, out = ctx.select_multi(dev, m, x, out=mine)
        assert out is mine and (rc, cnt, tot) == (0, n_w, t_w) and mine.n_words == n_w
        assert mine.download().tobytes() == rec_w.tobytes()
        mine.free()
    rc_w, n_w, t_w, rec_w = model(("sizes", n, 3 * SU.select_tile() + 17), lists, 1, n, 1, 0, 1)
    small = ctx.alloc(n_w - 1, 25)
    with pytest.raises(capi.Gt4HipError) as e:
        ctx.select_multi(dev, 1, n, out=small)
    assert e.value.code == capi.EINVAL and "capacity" in str(e.value)
    small.free()
    for l, d in zip(lists, dev):  # the inputs are only read
        assert d.download().tobytes() == l.tobytes()
        d.free()


@pytest.mark.parametrize("n", [2, 8, 9, 32])
def test_table_select_on_a_ragged_table_and_on_the_same_table_compacted(ctx, n):
    size = 3 * SU.nway_tile() + 17
    lists = make_lists(n, size)
    dev = [ctx.upload(l, 25) for l in lists]
    table = ctx.device_table(dev)
    assert table.ragged and (table.n_keys, table.n_lists) == (size, n)
    cases = [(m, x, cutoff, rule, ovr) for m, x in pairs(n) for cutoff, rule, ovr in [(1, ADD, 1), (3, MAX, 1), (2, NUMBER, 2)]]
    ragged = []
    for m, x, cutoff, rule, ovr in cases:
        rc, cnt, tot, out = ctx.table_select(table, m, x, cutoff, rule, ovr)
        rc_w, n_w, t_w, rec_w = model(("sizes", n, size), lists, m, x, cutoff, rule, ovr)
        ragged.append(out.download().tobytes())
        assert (rc, cnt, tot) == (0, n_w, t_w) and ragged[-1] == rec_w.tobytes()
        assert ctx.table_select(table, m, x, cutoff, rule, ovr, count_only=True) == (0, n_w, t_w, None)
        out.free()
    keys, counts = table.download()
    table.compact()
    assert not table.ragged and table.n_keys == size
    for (m, x, cutoff, rule, ovr), want in zip(cases, ragged):
        rc, cnt, tot, out = ctx.table_select(table, m, x, cutoff, rule, ovr)
        assert out.download().tobytes() == want and cnt * 12 == len(want)
        out.free()
    keys2, counts2 = table.download()  # the table is left as it was
    assert np.array_equal(keys, keys2) and np.array_equal(counts, counts2)
    table.free()
    for d in dev:
        d.free()


@pytest.mark.parametrize("n", [4, 8, 12, 32, 36, 68, 260])
def test_rows_of_a_multiple_of_four_counts_in_both_load_widths(ctx, n):
    """such rows are read 16 bytes per lane (counter "select_wide"); option "select_vec" = -1 reads them a dword per lane, as
    every other row is read: the same records either way, on the ragged and on the contiguous table"""
    size = SU.nway_tile() + SU.select_tile() + 3
    lists = make_lists(n, size)
    dev = [ctx.upload(l, 25) for l in lists]
    table = ctx.device_table(dev)
    assert table.ragged == (n <= 32)
    try:
        for form in ("as built", "compacted"):
            if form == "compacted":
                table.compact()
            for m, x in pairs(n):
                for cutoff, rule, ovr in [(1, ADD, 1), (3, MAX, 1)]:
                    rc_w, n_w, t_w, rec_w = model(("sizes", n, size), lists, m, x, cutoff, rule, ovr)
                    for vec, wide in ((0, 1), (-1, 0)):
                        ctx.set_option("select_vec", vec)
                        rc, cnt, tot, out = ctx.table_select(table, m, x, cutoff, rule, ovr)
                        assert ctx.get_counter("select_wide") == wide
                        assert (rc, cnt, tot) == (0, n_w, t_w) and out.download().tobytes() == rec_w.tobytes(), (n, form, m, x, vec)
                        out.free()
    finally:
        ctx.set_option("select_vec", 0)
    table.free()
    for d in dev:
        d.free()
    odd = [ctx.upload(l, 25) for l in make_lists(9, 100)]
    ctx.select_multi(odd, 1, 9)[3].free()
    assert ctx.get_counter("select_wide") == 0
    for d in odd:
        d.free()


def test_table_select_on_a_table_of_seventy_lists(ctx):
    n, size = 70, 3 * SU.select_segment() + 17
    lists = make_lists(n, size)
    dev = [ctx.upload(l, 25) for l in lists]
    table = ctx.device_table(dev)
    assert not table.ragged and (table.n_keys, table.n_lists) == (size, n)  # more than 32 lists: by merges
    for m, x in pairs(n):
        for cutoff, rule, ovr in [(1, ADD, 1), (3, MAX, 1)]:
            rc_w, n_w, t_w, rec_w = model(("sizes", n, size), lists, m, x, cutoff, rule, ovr)
            mine = ctx.alloc(n_w + 1, 25)
            rc, cnt, tot, out = ctx.table_select(table, m, x, cutoff, rule, ovr, out=mine)
            assert (rc, cnt, tot) == (0, n_w, t_w) and mine.download().tobytes() == rec_w.tobytes() and mine.word_length == 25
            mine.free()
    table.free()
    for d in dev:
        d.free()


@pytest.mark.parametrize("n", N_LISTS)
@pytest.mark.parametrize("rule,ovr,cutoff", [(0, 1, 1), (MAX, 1, 3), (NUMBER, 3, 1)])
def test_everything_selected_is_union_multi(ctx, n, rule, ovr, cutoff):
    lists = make_lists(n, 3 * SU.select_tile() + 17)
    dev = [ctx.upload(l, 25) for l in lists]
    rc, cnt, tot, out = ctx.select_multi(dev, 1, n, cutoff, rule, ovr)
    rc_u, cnt_u, tot_u, union = ctx.union_multi(dev, cutoff, rule, ovr)
    assert (rc, cnt, tot) == (rc_u, cnt_u, tot_u) == (0,) + O.union_multi(lists, cutoff, rule, ovr)[1:3]
    assert out.download().tobytes() == union.download().tobytes()
    rc, cnt, tot, core = ctx.select_multi(dev, n, n)
    rc_i, cnt_i, tot_i, inter = ctx.intersect_multi(dev)
    assert cnt == cnt_i and np.array_equal(core.download()["key"], inter.download()["key"])
    for d in dev + [out, union, core, inter]:
        d.free()


def test_bad_bounds_and_refused_rules(ctx):
    lists = make_lists(3, 100)
    dev = [ctx.upload(l, 25) for l in lists]
    for m, x in [(4, 4), (0, 2), (0, 0), (3, 2), (1, 4), (2, 1)]:
        with pytest.raises(capi.Gt4HipError) as e:
            ctx.select_multi(dev, m, x)
        assert e.value.code == capi.EINVAL and "min_lists %d, max_lists %d" % (m, x) in str(e.value)
    table = ctx.device_table(dev)
    with pytest.raises(capi.Gt4HipError) as e:
        ctx.table_select(table, 1, 4)
    assert e.value.code == capi.EINVAL and "3 lists" in str(e.value)
    for rule in (capi.RULE_SUBTRACT, capi.RULE_MIN, capi.RULE_FIRST, capi.RULE_SECOND):
        assert ctx.select_multi(dev, 1, 3, rule=rule)[0] == capi.ERULE
        assert ctx.table_select(table, 1, 3, rule=rule)[0] == capi.ERULE
        assert ctx.union_multi(dev, rule=rule)[0] == capi.ERULE
    table.free()
    with pytest.raises(capi.Gt4HipError) as e:
        ctx.select_multi(dev[:2] + [ctx.upload(lists[2], 24)], 1, 3)
    assert e.value.code == capi.EWORDLEN
    for d in dev:
        d.free()
