"""The two persistent merge kernels, k_nway_merge (gt4hip_nway_tile.h) and k_pair_merge (gt4hip_kernels.hip), run with a
handful of workgroups, so that every worker takes tile after tile and everything it carries from one tile to the next is
used many times over: the three rotating slot / run tables, the ticket drawn three tiles ahead, the records prefetched one
tile ahead, the leader bitmap of alternating parity, the staged output written out in the middle of the next tile
(write_out, resolve_offset), fill_g between tiles, and the count tables' LDS row area, which only "every thread zeroes the
16 bytes it has just sent out" keeps clean behind the first tile.  At the default grid (one workgroup per CU) the inputs of
the other N-way tests give a workgroup one tile, which touches none of that.

Every case runs its call at the default grid and then under option "grid" = g with both dealings ("dynamic" = -1 and 1:
round-robin and by ticket), and asserts: the bytes of the CPU reference (oracle_lib.union_multi / oracle_lib.compare, a
numpy count table); the bytes of the default-grid run; that the tile kernel did the work (counters "kway_calls",
"single_pass_fallbacks", "kway_declined", "kway_overflows", "nway_one_pass", the ragged table); and, by counter
("nway_tiles", "nway_sample_tiles", the pair call's merge_tiles), that the launch under test had at least eight tiles per
worker -- workers being g - 1 where a launch has a scanner workgroup (a union that writes records, the single-pass pair
kernel; "grid" = 1 gives such a launch two workgroups) and g elsewhere.  The short-loop cases state the exact number of tiles
they are about instead.  Each run prints a line with its tile counts (pytest -s; profiles/few_workers/README.md).

The module's context runs with option "poison" (a pooled block must not hand the run under test the results of the run before)
and "kway" = 3 (the tile kernel whatever the keys)."""
import numpy as np
import pytest

import oracle_lib as O
import pair_variants as V
import select_util as SU
from genometester4_amd import capi
from genometester4_amd.listio import make_records
from test_kway import _random_lists
from test_pair_variants import C_EDGE, _universe_pair
from test_select_gpu import make_lists

pytestmark = pytest.mark.gpu

ADD, MAX, NUMBER, FIRST = capi.RULE_ADD, capi.RULE_MAX, capi.RULE_NUMBER, capi.RULE_FIRST
U32 = 0xFFFFFFFF
MIN_PER_WORKER = 8
RESET = {"grid": 0, "dynamic": 0, "scan_group": 0, "kway_g": 0, "kway_vt": 0, "kway_max": 32, "two_pass": 0}
UNION_GRIDS = (1, 2, 3, 4)   # a union that writes records: the scanner workgroup and g - 1 workers (g = 1: as g = 2)
OTHER_GRIDS = (1, 2, 3)      # count-only calls and count tables: g workers
ROWW = SU._define("gt4hip_nway_tile.h", "GT4_NWAY_ROWW")   # words of the count tables' row area in LDS
TILE = SU.nway_tile()                                       # positions of a tile
SAMPLE = {8: SU._define("gt4hip_nway_part.h", "GT4_NWAY_SAMPLE"), 32: 64}  # records a sample stands for, by instance
RUN_PAD = {8: 64, 32: 1}                                    # a run is rounded up to this many positions (NWAY_HS)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    c.set_option("poison", 1)
    c.set_option("kway", 3)
    yield c
    c.close()


def _under(ctx, opts, fn):
    """fn () under the options, every one of them reset whatever happens"""
    try:
        for name, value in opts.items():
            ctx.set_option(name, value)
        return fn()
    finally:
        for name in opts:
            ctx.set_option(name, RESET[name])


# ------------------------------------------------------------------ inputs (CPU only: no context, no library)

def one_tile_records(n_lists, inst):
    """records that fit one tile whatever they are (nway_run: one_tile): a call with more has sample levels"""
    return TILE - RUN_PAD[inst] * n_lists


def auto_g(n_lists, inst):
    """samples per tile of the first partition attempt (nway_samples_per_tile: the expected tile plus five standard deviations)"""
    s, pad = SAMPLE[inst], RUN_PAD[inst]
    g1 = int((TILE - 0.5 * pad * n_lists - 5.0 * s * (n_lists / 6.0) ** 0.5) / s)
    g0 = max((TILE - pad * n_lists) // s - (2 * n_lists - 1), 1)
    return max(g1, g0)


def level_tiles(sizes, inst, g):
    """tiles of the launch over lists of these sizes cut at every g-th merged sample of the level above, before any tile
    is cut in two (nway_partition_level: samples above / G + 2; one tile where the lists fit one)"""
    if sum(sizes) <= one_tile_records(len(sizes), inst):
        return 1
    return sum(n // SAMPLE[inst] for n in sizes) // g + 2


def wrap_lists(seed, n_lists, universe, k_bits=40):
    """random lists with zero counts; every 40th key is held by lists 0 and 1 alone with counts whose sum is 2^32 (ADD wraps
    to exactly 0), every 40th + 1 with a sum of 2^32 + 1 (wraps to 1)"""
    rng = np.random.default_rng(seed)
    keys = np.unique(rng.integers(0, 1 << k_bits, size=universe, dtype=np.uint64))
    kind = np.zeros(len(keys), dtype=np.int64)
    kind[5::40] = 1
    kind[6::40] = 2
    frac = np.linspace(0.15, 0.9, n_lists)
    lists = []
    for j in range(n_lists):
        m = rng.random(len(keys)) < frac[(5 * j) % n_lists]
        m[kind > 0] = j < 2
        c = rng.integers(0, 7, size=len(keys), dtype=np.uint32)
        c[kind == 1] = U32 if j == 0 else 1
        c[kind == 2] = U32 if j == 0 else 2
        lists.append(make_records(keys[m], c[m]))
    return lists, keys[kind == 1], keys[kind == 2]


def check_wraps(lists, to_zero, to_one):
    """the oracle's ADD at cutoff 0 holds at least 1,000 keys whose sum wrapped to 0 and 1,000 to 1"""
    rc, n, t, rec = O.union_multi(lists, 0, ADD, 1)
    assert rc == 0 and len(to_zero) >= 1000 and len(to_one) >= 1000
    assert np.all(rec["count"][np.searchsorted(rec["key"], to_zero)] == 0)
    assert np.all(rec["count"][np.searchsorted(rec["key"], to_one)] == 1)
    assert int((rec["count"] == 0).sum()) >= 1000 and int((rec["count"] == 1).sum()) >= 1000


def high_cutoff(lists, rule):
    """a cutoff above most folded counts: the 90 % quantile of the oracle's counts at cutoff 0; at least 1,000 keys stay
    below it and at least 1,000 reach it (k_nway_merge's `drop` gives the leader bits of the former back)"""
    rc, n, t, rec = O.union_multi(lists, 0, rule, 1)
    assert rc == 0
    hi = max(int(np.quantile(rec["count"], 0.9)), 3)
    below, reach = int((rec["count"] < hi).sum()), int((rec["count"] >= hi).sum())
    assert below >= 1000 and reach >= 1000, (rule, hi, below, reach)
    return hi


def number_cutoffs(lists, ovr=3):
    """NUMBER gives every key the count `ovr`, so no cutoff splits the keys: the oracle keeps every distinct key at cutoff
    ovr - 1 and none at ovr + 1 (every leader bit is given back); returns the two cutoffs"""
    distinct = len(np.unique(np.concatenate([x["key"] for x in lists])))
    rc, n, t, rec = O.union_multi(lists, ovr - 1, NUMBER, ovr)
    assert rc == 0 and n == distinct >= 1000 and t == ovr * distinct
    rc, n, t, rec = O.union_multi(lists, ovr + 1, NUMBER, ovr)
    assert rc == 0 and n == 0 and t == 0
    return ovr - 1, ovr + 1


def mixed_lists(seed=31):
    """test_kway.test_clustered_keys' second input: one dense run inside uniform keys, so that the tiles around the run take
    the search path and their neighbours on the same worker do not"""
    rng = np.random.default_rng(seed)
    uni = np.unique(rng.integers(0, 1 << 50, size=200000, dtype=np.uint64))
    dense = np.arange(1 << 49, (1 << 49) + 30000, dtype=np.uint64)
    lists = []
    for j in range(4):
        k = np.unique(np.concatenate([uni[rng.random(len(uni)) < 0.6], dense[rng.random(len(dense)) < 0.7]]))
        lists.append(make_records(k, rng.integers(1, 9, size=len(k), dtype=np.uint32)))
    for x in lists:  # the clustered stretch and the uniform one, each many tiles long
        gap = np.diff(x["key"])
        inside = (x["key"][:-1] >= 1 << 49) & (x["key"][1:] < (1 << 49) + 30000)
        assert int(inside.sum()) >= 4 * TILE and gap[inside].max() <= 64
        assert int((~inside).sum()) >= 20 * TILE and np.median(gap[~inside]) > 1 << 30
    return lists


def narrow_and_wide_lists(seed=41, stretches=10, per_stretch=16000):
    """stretches of keys by turns spread over 2^50 (a tile spans far more than 2^32: 8-byte keys) and over 2^26 (a tile
    spans less than 2^32: 4-byte keys relative to the tile's smallest), each several tiles long"""
    rng = np.random.default_rng(seed)
    parts = []
    for s in range(stretches):
        span = 1 << (50 if s % 2 == 0 else 26)
        parts.append((np.uint64(s) << np.uint64(52)) + rng.integers(0, span, size=per_stretch, dtype=np.uint64))
    keys = np.unique(np.concatenate(parts))
    lists = []
    for j in range(5):
        m = rng.random(len(keys)) < (0.9 if j < 3 else 0.4)
        lists.append(make_records(keys[m], rng.integers(0, 7, size=int(m.sum()), dtype=np.uint32)))
    for s in range(stretches):  # on the keys themselves: every stretch several tiles long, narrow ones below 2^32, wide ones far above
        lo, hi = np.uint64(s) << np.uint64(52), np.uint64(s + 1) << np.uint64(52)
        part = [x["key"][(x["key"] >= lo) & (x["key"] < hi)] for x in lists]
        assert sum(len(k) for k in part) >= 3 * TILE and min(len(k) for k in part) >= TILE
        for k in part:
            span = int(k[-1]) - int(k[0])
            if s % 2:
                assert span < 1 << 32
            else:  # a tile's share of this list (a fifth of a tile's records at the least) spans more than 2^32
                assert np.median(np.diff(k)) * (TILE // 5) > 1 << 36 and span > 1 << 48
    return lists


def disjoint_lists(seed=9):
    """list j owns keys [j * 2^30, (j + 1) * 2^30): every tile but those at the seams holds one list only"""
    rng = np.random.default_rng(seed)
    lists = []
    for j in range(6):
        k = np.unique(rng.integers(j << 30, (j + 1) << 30, size=40000 + 7000 * j, dtype=np.uint64))
        lists.append(make_records(k, rng.integers(1, 9, size=len(k), dtype=np.uint32)))
    return lists


def skewed_lists(seed, n_lists, universe):
    """list 0 holds 85 % of the keys, every other list 5 %: most rows of a count table have one count, and list 0 is most of
    every tile -- the rows of a tile, of the union and of list 0 alike, need more than one batch of the LDS row area"""
    rng = np.random.default_rng(seed)
    keys = np.unique(rng.integers(0, 1 << 44, size=universe, dtype=np.uint64))
    lists = []
    for j in range(n_lists):
        m = rng.random(len(keys)) < (0.85 if j == 0 else 0.05)
        lists.append(make_records(keys[m], rng.integers(0, 7, size=int(m.sum()), dtype=np.uint32)))
    return lists


def same_key_lists(seed, n_lists, n_keys):
    """every list holds every key: a tile has at most TILE / n_lists rows, which fit one batch of the row area"""
    rng = np.random.default_rng(seed)
    keys = np.unique(rng.integers(0, 1 << 44, size=n_keys, dtype=np.uint64))
    assert TILE // n_lists <= ROWW // n_lists
    return [make_records(keys, rng.integers(0, 7, size=len(keys), dtype=np.uint32)) for _ in range(n_lists)]


def exact_lists(seed, sizes, k_bits=40):
    """lists of exactly these lengths out of one universe"""
    rng = np.random.default_rng(seed)
    keys = np.unique(rng.integers(0, 1 << k_bits, size=2 * max(sizes) + 16, dtype=np.uint64))
    lists = []
    for n in sizes:
        k = np.sort(rng.choice(keys, size=n, replace=False))
        lists.append(make_records(k, rng.integers(0, 7, size=n, dtype=np.uint32)))
    return lists


def rows_need_batches(lists, tiles, probe):
    """pigeonhole: the table's rows (probe: list 0's records) over `tiles` tiles are more than one batch each on average, so
    at least one tile needs a second batch"""
    rows = len(lists[0]) if probe else len(np.unique(np.concatenate([x["key"] for x in lists])))
    return rows > tiles * (ROWW // len(lists))


# ------------------------------------------------------------------ references

def np_table(lists, probe=False, presence=False):
    """np.unique over all keys; column j: list j's count of the key (presence: 1) or 0; probe: the rows of list 0"""
    uni = np.unique(np.concatenate([x["key"] for x in lists]))
    tab = np.zeros((len(uni), len(lists)), dtype=np.uint32)
    for j, x in enumerate(lists):
        tab[np.searchsorted(uni, x["key"]), j] = 1 if presence else x["count"]
    if probe:
        rows = np.searchsorted(uni, lists[0]["key"])
        uni, tab = uni[rows], tab[rows]
    return uni.tobytes(), np.ascontiguousarray(tab).tobytes()


TABLE_KINDS = {"table": {}, "table_compact": {"compact": True}, "probe": {"probe": True},
               "presence": {"probe": True, "presence": True}}


def reference(kind, lists, args):
    if kind in TABLE_KINDS:
        kw = TABLE_KINDS[kind]
        return np_table(lists, kw.get("probe", False), kw.get("presence", False))
    cutoff, rule, ovr = args
    rc, n, t, rec = O.union_multi(lists, cutoff, rule, ovr)
    assert rc == 0
    return (n, t, None if kind == "count" else rec.tobytes())


# ------------------------------------------------------------------ the helper: one call under few workers

COUNTERS = ("kway_calls", "single_pass_fallbacks", "kway_declined", "kway_overflows")


def run_nway(ctx, dev, kind, args, opts):
    """one N-way call under the options: (result, tiles of the last launch, most tiles of a sample-level launch); asserts that
    the tile kernel did the work and that no wait gave up"""
    before = {c: ctx.get_counter(c) for c in COUNTERS}

    def call():
        if kind in TABLE_KINDS:
            keys, counts = ctx.union_table(dev, **TABLE_KINDS[kind])
            return keys.tobytes(), counts.tobytes()
        cutoff, rule, ovr = args
        rc, n, t, out = ctx.union_multi(dev, cutoff, rule, ovr, kind == "count")
        assert rc == 0
        if out is None:
            return n, t, None
        got = out.download().tobytes()
        out.free()
        return n, t, got

    got = _under(ctx, opts, call)
    after = {c: ctx.get_counter(c) for c in COUNTERS}
    assert after["kway_calls"] == before["kway_calls"] + 1, (kind, opts)
    for c in COUNTERS[1:]:
        assert after[c] == before[c], (c, kind, opts)
    if kind in ("union", "count"):
        assert ctx.get_counter("nway_one_pass") == 1
    if kind in ("table", "table_compact"):
        assert ctx.last_table_was_ragged
    return got, ctx.get_counter("nway_tiles"), ctx.get_counter("nway_sample_tiles")


def workers_of(kind, g):
    return max(g, 2) - 1 if kind == "union" else g


def sweep(ctx, name, lists, k, kind, args=(1, 0, 1), grids=None, opts=None, dynamics=(-1, 1), scan_groups=(0,),
          exact_tiles=None, sample_level=False, ref=None, also=None):
    """the call at the default grid, then under every (grid, dealing, scanner): the reference's bytes, the default-grid run's
    bytes, and a long loop -- at least MIN_PER_WORKER tiles per worker (exact_tiles: exactly that many tiles in the
    launch instead; sample_level: the sample-level launches too).  also (ctx): further assertions behind every run.
    Returns the tile counts seen."""
    opts = dict(opts or {})
    grids = grids if grids is not None else (UNION_GRIDS if kind == "union" else OTHER_GRIDS)
    ref = ref if ref is not None else reference(kind, lists, args)
    dev = [ctx.upload(x, k) for x in lists]
    seen = set()
    try:
        base, tiles0, st0 = run_nway(ctx, dev, kind, args, opts)
        assert base == ref, (name, kind, args, "default grid")
        if also:
            also(ctx)
        for g in grids:
            for dyn in dynamics:
                for sg in scan_groups:
                    o = dict(opts, grid=g, dynamic=dyn, scan_group=sg)
                    got, tiles, stiles = run_nway(ctx, dev, kind, args, o)
                    w = workers_of(kind, g)
                    print("few_workers %s %s args=%s g=%d dynamic=%d scan_group=%d: tiles %d workers %d sample_tiles %d"
                          % (name, kind, args, g, dyn, sg, tiles, w, stiles))
                    assert got == ref, (name, kind, args, o)
                    assert got == base, (name, kind, args, o)
                    assert (tiles, stiles) == (tiles0, st0)
                    if also:
                        also(ctx)
                    if exact_tiles is not None:
                        assert tiles == exact_tiles, (name, tiles, exact_tiles)
                    else:
                        assert tiles >= MIN_PER_WORKER * w, (name, tiles, w)
                    if sample_level:
                        assert stiles >= MIN_PER_WORKER * g, (name, stiles, g)  # (a sample level has no scanner: g workers)
                    seen.add(tiles)
    finally:
        for d in dev:
            d.free()
    return seen


def width_is(w):
    def check(ctx):
        assert ctx.get_counter("kway_width") == w
    return check


# the two instances of the tile kernel: up to eight lists, and up to 32 (twelve lists go there under "kway_max" = 33)
INSTANCES = {"8": (8, {}, 8), "12in32": (12, {"kway_max": 33}, 32)}

# ------------------------------------------------------------------ NWAY_UNION and NWAY_COUNT

_wrap_cache = {}


def _wrap_input(inst):
    if inst not in _wrap_cache:
        n_lists = INSTANCES[inst][0]
        lists, z, o = wrap_lists(100 + n_lists, n_lists, 90000 if n_lists == 8 else 60000)
        assert 300_000 <= sum(len(x) for x in lists) <= 1_100_000
        check_wraps(lists, z, o)
        _wrap_cache[inst] = lists
    return _wrap_cache[inst]


@pytest.mark.parametrize("inst", list(INSTANCES))
@pytest.mark.parametrize("rule,ovr", [(ADD, 1), (MAX, 1), (NUMBER, 3)], ids=["add", "max", "number3"])
def test_union_and_count_rules_and_cutoffs(ctx, inst, rule, ovr):
    """rules ADD, MAX, NUMBER over lists with zero counts and ADD sums that wrap to exactly 0 and 1, at the automatic samples
    per tile (full tiles); cutoffs 0, 2 and one above most folded counts.  (NUMBER gives every key the same count, 3:
    cutoff 2 keeps every key, cutoff 4 drops every key and gives every leader bit back.)"""
    n_lists, opts, width = INSTANCES[inst]
    lists = _wrap_input(inst)
    hi = number_cutoffs(lists, ovr)[1] if rule == NUMBER else high_cutoff(lists, rule)
    for cutoff in (0, 2, hi):
        ref = reference("union", lists, (cutoff, rule, ovr))
        sweep(ctx, "rules-" + inst, lists, 20, "union", (cutoff, rule, ovr), opts=opts, ref=ref, also=width_is(width))
        sweep(ctx, "rules-" + inst, lists, 20, "count", (cutoff, rule, ovr), opts=opts, ref=ref[:2] + (None,), also=width_is(width))


def test_union_and_count_of_thirty_two_lists(ctx):
    """32 real lists that share little: one launch of the 32-list instance on its own account"""
    rng = np.random.default_rng(32)
    keys = np.unique(rng.integers(0, 1 << 44, size=150000, dtype=np.uint64))
    lists = []
    for j in range(32):
        m = rng.random(len(keys)) < (0.03 if j % 3 else 0.25)
        lists.append(make_records(keys[m], rng.integers(0, 9, size=int(m.sum()), dtype=np.uint32)))
    assert 300_000 <= sum(len(x) for x in lists) <= 1_100_000
    for kind in ("union", "count"):
        sweep(ctx, "lists32", lists, 22, kind, (2, ADD, 1), also=width_is(32))


# ------------------------------------------------------------------ NWAY_DUPS: the sample levels

LEVEL_CASES = [("8", 260000, 2), ("12in32", 75000, 3)]  # instance, universe, samples per tile


def sample_level_lists(inst, universe, g):
    """lists with two sample levels whose level-1 launch has at least eight tiles per worker at g samples per tile"""
    n_lists, _, width = INSTANCES[inst]
    rng = np.random.default_rng(7 + n_lists)
    lists = _random_lists(rng, n_lists, universe)
    sizes = [len(x) for x in lists]
    assert sum(sizes) <= 1_100_000
    level1 = [n // SAMPLE[width] for n in sizes]
    level2 = [n // SAMPLE[width] for n in level1]
    assert sum(level1) > one_tile_records(n_lists, width) >= sum(level2)       # levels 1 and 2, and no third
    assert level_tiles(level1, width, g) >= MIN_PER_WORKER * max(OTHER_GRIDS)  # the launch over level 1
    return lists


@pytest.mark.parametrize("inst,universe,g", LEVEL_CASES)
@pytest.mark.parametrize("kind", ["union", "table"])
def test_sample_levels(ctx, inst, universe, g, kind):
    """two sample levels, few samples per tile ("kway_g"): the launch over level 1 (NWAY_DUPS, merged samples that keep their
    list numbers) has at least eight tiles per worker as well, by counter "nway_sample_tiles" """
    n_lists, opts, width = INSTANCES[inst]
    lists = sample_level_lists(inst, universe, g)
    grids = (1, 2, 3)  # (a union's last launch: a scanner and 1, 1, 2 workers; its sample level: 1, 2, 3 workers)
    sweep(ctx, "levels-" + inst, lists, 20, kind, (1, ADD, 1), grids=grids, opts=dict(opts, kway_g=g), sample_level=True)


# ------------------------------------------------------------------ NWAY_TABLE and NWAY_PROBE

_table_cache = {}


def _table_input(name, n_lists):
    key = (name, n_lists)
    if key not in _table_cache:
        _table_cache.clear()
        if name == "select":   # word i in 1 + (i mod n) lists drawn at random: keys of list 0 alone, keys list 0 lacks
            size = {3: 170000, 8: 80000, 12: 60000}[n_lists]
            lists = make_lists(n_lists, size, seed=3, zero_counts=True)
            only0 = np.setdiff1d(lists[0]["key"], np.concatenate([x["key"] for x in lists[1:]]))
            not0 = np.setdiff1d(np.concatenate([x["key"] for x in lists[1:]]), lists[0]["key"])
            assert len(only0) >= 100 and len(not0) >= 100
        elif name == "skewed":
            lists = skewed_lists(50 + n_lists, n_lists, {3: 330000, 8: 300000, 12: 260000, 32: 170000}[n_lists])
        else:
            lists = same_key_lists(60 + n_lists, n_lists, 400000 // n_lists)
        assert 300_000 <= sum(len(x) for x in lists) <= 1_100_000, (name, n_lists, sum(len(x) for x in lists))
        _table_cache[key] = lists
    return _table_cache[key]


TABLE_CASES = [(n, name) for n in (3, 8, 12) for name in ("select", "skewed", "same")] + [(32, "skewed")]


@pytest.mark.parametrize("kind", ["table", "probe", "presence"])
@pytest.mark.parametrize("n_lists,name", TABLE_CASES, ids=["%d-%s" % c for c in TABLE_CASES])
def test_count_tables(ctx, n_lists, name, kind):
    """the count table, and the tables of list 0's keys with counts and with presence.  "skewed": tiles whose rows need more
    than one batch of the LDS row area (ROWW / columns rows: 1,792 at eight columns) -- the second batch lies where the first
    was sent from; "same": every tile's rows fit one batch; "select": keys that list 0 alone holds, and keys it lacks"""
    lists = _table_input(name, n_lists)
    width = 8 if n_lists <= 8 else 32
    many = name == "skewed" and n_lists >= 8
    if many:  # (by the tiles the partition starts from; below: by the tiles the launch had)
        assert rows_need_batches(lists, level_tiles([len(x) for x in lists], width, auto_g(n_lists, width)), kind != "table")
    if name == "same":
        assert TILE // n_lists <= ROWW // n_lists
    seen = sweep(ctx, "table-%s-%d" % (name, n_lists), lists, 25, kind)
    if n_lists == 8 and name == "select" and kind == "table":
        sweep(ctx, "table-%s-%d" % (name, n_lists), lists, 25, "table_compact", grids=(2,))
    if many:
        assert rows_need_batches(lists, max(seen), kind != "table"), (n_lists, kind, seen)


# ------------------------------------------------------------------ the tile paths

def _path_case(path):
    """(lists, k, options, what to assert behind every run)"""
    if path in ("vt99", "vt98"):  # every tile on the search path / bucketed by its pivot run
        rng = np.random.default_rng(4242)
        return _random_lists(rng, 8, 90000), 20, {"kway_vt": int(path[2:])}, None
    if path == "mixed":
        return mixed_lists(), 25, {}, None
    if path == "narrow_wide":
        return narrow_and_wide_lists(), 32, {}, None
    if path == "disjoint":
        return disjoint_lists(), 20, {}, None

    def cut(ctx):
        assert ctx.get_counter("kway_splits") > 0
    if path == "cut8":   # more samples per tile than fit on average: about half of the tiles are cut in two
        rng = np.random.default_rng(30)
        return _random_lists(rng, 8, 150000, zero_counts=False), 20, {"kway_g": 30}, cut
    assert path == "cut12"
    rng = np.random.default_rng(12)
    return _random_lists(rng, 12, 110000, zero_counts=False), 20, {"kway_g": 64, "kway_max": 33}, cut


@pytest.mark.parametrize("path", ["vt99", "vt98", "mixed", "narrow_wide", "disjoint", "cut8", "cut12"])
@pytest.mark.parametrize("kind", ["union", "table"])
def test_tile_paths(ctx, path, kind):
    """the paths a tile can take, with consecutive tiles of one worker on different ones"""
    lists, k, opts, also = _path_case(path)
    assert 300_000 <= sum(len(x) for x in lists) <= 1_100_000, sum(len(x) for x in lists)
    sweep(ctx, "path-" + path, lists, k, kind, (1, ADD, 1), opts=opts, also=also)


# ------------------------------------------------------------------ the scanner as summers + chainer

SCAN_G = 4  # samples per tile of the scanner cases: four lists of 128 q + 5 records have 4 q samples above, q + 2 tiles


@pytest.mark.parametrize("tiles", [1, 63, 64, 65, 8 * 64 + 10])
def test_scanner_group_of_the_tile_kernel(ctx, tiles):
    """ "scan_group" = 1 on unions whose last launch has 1, 63, 64, 65 and more than 8 x 64 tiles: a row of 64 tiles short of
    one, full, and with one tile in the next row; more rows than the eight summers.  At the default grid and with two
    workers; the largest also with "scan_group" = -1 (the single wavefront)."""
    q = tiles - 2
    sizes = [SAMPLE[8] * q + 5] * 4 if tiles > 1 else [700, 800, 900, 1000]
    assert level_tiles(sizes, 8, SCAN_G) == tiles
    lists = exact_lists(tiles, sizes)
    ref = reference("union", lists, (1, ADD, 1))
    dev = [ctx.upload(x, 20) for x in lists]
    try:
        for sg in (1, -1) if tiles > 8 * 64 else (1,):
            for g in (0, 3):
                for dyn in (-1, 1) if g else (0,):
                    o = {"kway_g": SCAN_G, "scan_group": sg, "grid": g, "dynamic": dyn}
                    got, n_tiles, _ = run_nway(ctx, dev, "union", (1, ADD, 1), o)
                    print("few_workers scanner union g=%d dynamic=%d scan_group=%d: tiles %d" % (g, dyn, sg, n_tiles))
                    assert n_tiles == tiles
                    assert got == ref, o
    finally:
        for d in dev:
            d.free()


# ------------------------------------------------------------------ short loops

# three lists with 28 samples above them and more records than one tile holds: 28 / G + 2 tiles
SHORT_SIZES = (1407, 1407, 1151)
SHORT_G = {2: 30, 3: 20, 4: 12, 5: 8, 6: 7}


@pytest.mark.parametrize("kind", ["union", "table"])
def test_short_loops_of_the_tile_kernel(ctx, kind):
    """exactly 1 .. 6 tiles in the launch, on one worker and on two: the prologue's four deals (of which some find no tile),
    the table built two tiles ahead for a tile that does not exist, the prefetch that has nothing to fetch, the drain"""
    assert sum(n // SAMPLE[8] for n in SHORT_SIZES) == 28 and sum(SHORT_SIZES) > one_tile_records(3, 8)
    seen = set()
    for tiles in range(1, 7):
        sizes = SHORT_SIZES if tiles > 1 else (1300, 1300, 1100)
        opts = {"kway_g": SHORT_G[tiles]} if tiles > 1 else {}
        assert level_tiles(sizes, 8, SHORT_G.get(tiles, 24)) == tiles
        lists = exact_lists(10 + tiles, sizes)
        grids = (2, 3) if kind == "union" else (1, 2)  # one worker, two workers
        seen |= sweep(ctx, "short-%d" % tiles, lists, 20, kind, (1, ADD, 1), grids=grids, opts=opts, exact_tiles=tiles)
    assert seen == {1, 2, 3, 4, 5, 6}


# ------------------------------------------------------------------ the pair kernel

PAIR_CALLS = [(1, 0, 0), (2, 0, 0), (4, 0, 0), (8, 0, 0), (3, 0, 0), (15, 0, 0), (15, MAX, 0), (2, FIRST, 0), (5, 0, 1)]
# path: (options, count_only, grids).  The default path's launch has a scanner (MODE_LOOKBACK: g - 1 workers, g = 1 as g = 2);
# the two-pass path's two launches (MODE_COUNT, MODE_OFFSETS) and the count-only launch have none.
PAIR_PATHS = {"default": ({}, False, (1, 2, 3)), "two_pass": ({"two_pass": 1}, False, (1, 2)), "count_only": ({}, True, (1, 2))}


@pytest.fixture(scope="module")
def pair(ctx):
    a, b = _universe_pair(23, 25, 300000)
    assert 180_000 <= len(a) <= 220_000 and 180_000 <= len(b) <= 220_000
    dev = (ctx.upload(a, 25), ctx.upload(b, 25))
    yield a, b, dev
    for d in dev:
        d.free()


def run_pair(ctx, a, b, dev, call, path, g, dyn, exp):
    """one gt4hip_compare under few workers against the oracle's result `exp`; returns the streams' bytes and the tiles"""
    ops, rule, sub = call
    opts, count_only, _ = PAIR_PATHS[path]
    before = ctx.get_counter("single_pass_fallbacks")
    st, out, timing = _under(ctx, dict(opts, grid=g, dynamic=dyn), lambda: ctx.compare(dev[0], dev[1], ops, rule, C_EDGE, sub, 1, count_only))
    assert ctx.get_counter("single_pass_fallbacks") == before, (call, path, g, dyn)
    launch = V.compare_launches(ops, rule, C_EDGE, sub, len(a), len(b), count_only=count_only, two_pass=bool(opts.get("two_pass")))
    assert timing["merge_tiles"] == launch.tiles
    got = {}
    for bit in (1, 2, 4, 8):
        if not ops & bit:
            continue
        assert st[bit] == exp[bit][:2], (call, path, g, dyn, bit)
        if not count_only:
            got[bit] = out[bit].download().tobytes()
            out[bit].free()
            assert got[bit] == exp[bit][2].tobytes(), (call, path, g, dyn, bit)
    return got, launch.tiles


@pytest.mark.parametrize("call", PAIR_CALLS, ids=["ops%d_rule%d_du%d" % c for c in PAIR_CALLS])
def test_pair_kernel(ctx, pair, call):
    """k_pair_merge in MODE_LOOKBACK (the default path), MODE_COUNT and MODE_OFFSETS (the two-pass path) and MODE_COUNT of the
    small geometry (count_only), every worker through at least eight tiles"""
    a, b, dev = pair
    ops, rule, sub = call
    exp = O.compare(a, b, ops, rule, C_EDGE, sub)
    for path, (_, _, grids) in PAIR_PATHS.items():
        base, _ = run_pair(ctx, a, b, dev, call, path, 0, 0, exp)
        for g in grids:
            for dyn in (-1, 1):
                got, tiles = run_pair(ctx, a, b, dev, call, path, g, dyn, exp)
                w = max(g, 2) - 1 if path == "default" else g
                print("few_workers pair ops=%d rule=%d du=%d %s g=%d dynamic=%d: tiles %d workers %d" % (ops, rule, sub, path, g, dyn, tiles, w))
                assert got == base
                assert tiles >= MIN_PER_WORKER * w


@pytest.mark.parametrize("ops", [1, 15])
def test_short_loops_of_the_pair_kernel(ctx, pair, ops):
    """1 .. 5 tiles on one worker: the ends of the three-deep ring (records of tile i + 1 in flight, the range of tile i + 2
    being read, the ticket of tile i + 3 being drawn) -- single pass (a scanner and one worker) and two-pass (one workgroup)"""
    a, b, _ = pair
    tile = V.merge_tile_records(1, ops)
    seen = set()
    for tiles in range(1, 6):
        n = (tiles * tile - 100) // 2
        sa, sb = a[:n].copy(), b[:n + 1].copy()
        exp = O.compare(sa, sb, ops, 0, C_EDGE, 0)
        dev = (ctx.upload(sa, 25), ctx.upload(sb, 25))
        try:
            for path, g in (("default", 2), ("two_pass", 1)):
                for dyn in (-1, 1):
                    _, n_tiles = run_pair(ctx, sa, sb, dev, (ops, 0, 0), path, g, dyn, exp)
                    print("few_workers pair-short ops=%d %s g=%d dynamic=%d: tiles %d workers 1" % (ops, path, g, dyn, n_tiles))
                    assert n_tiles == tiles
                    seen.add(n_tiles)
        finally:
            for d in dev:
                d.free()
    assert seen == {1, 2, 3, 4, 5}
