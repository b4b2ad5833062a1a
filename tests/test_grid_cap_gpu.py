"""Every kernel that walks its work in a loop stepping by gridDim.x, run with fewer workgroups than blocks of work.

A launcher gives such a kernel one workgroup per block of work up to a cap of thousands, so at the sizes of the other GPU
tests every workgroup makes one trip.  Option "grid_cap" = 1, 2, 3 cuts the grid; the inputs here have SEVEN blocks of work
for the kernel under test, once as six full blocks and one item (the last trip as partial as it can be) and once as seven
full blocks, so the workgroups make 3/2/2, 4/3 and 7 trips: uneven, and at least three for one of them.  Every case runs
the call uncapped, then capped, and asserts that counter "grid_capped" did not move in the first run and rose by at least
the number of striding launches of the call in the second, that the two outputs are byte-identical, and that the output is
the CPU model's by the comparison the family's own GPU test makes.  Block sizes come from counters of the library.  The
module's context runs with option "poison": without it the capped run finds the uncapped run's results in the pooled blocks
it reuses, and a loop whose stride skips an item passes (profiles/grid_cap/README.md).  Where a kernel of the call has more
blocks than the built-in cap whatever the input (level 2 of compare_mismatch), the uncapped run is cut there too and only
the capped run's count is asserted.

The sites (`gridDim\\.x` over genometester4_amd/csrc), their launcher, and the test that covers them:

  gt4hip_query.hip   k_query_exact                    gt4hip_grid  test_lookup_exact, test_index_build
                     k_query<false> (stride_r/_w)     gt4hip_grid  test_lookup_with_mismatches
                     k_query<true>                    gt4hip_grid  LEFT OUT: launched when variants + stride reach 2^32, which
                                                                   takes seven mismatches and more; seven blocks are 1792
                                                                   variants.  The loop and its carry are one text for both;
                                                                   tests/test_mismatch_depth_gpu.py runs the wide unranking
                     k_query_found                    gt4hip_grid  test_lookup_with_mismatches ["found-6+1", "found-7"]
                     k_query_hits<FILL, LOC>          gt4hip_grid  test_lookup_all (LOC = false), test_location_lookup (true)
                     k_index_split                    gt4hip_grid  test_location_index_create
                     k_gather_locations               gt4hip_grid  test_location_lookup
                     for_each_record: k_count_stats, k_count_split, k_count_histogram<LDS>, k_gc
                                                      gt4hip_grid  test_list_statistics
  gt4hip_index.h     k_index_build                    gt4hip_grid  test_index_build
                     k_tile_count                     gt4hip_grid  test_compare_mismatch
  gt4hip_mismatch.hip k_prepass, k_scatter, k_level<false>, k_decide
                                                      gt4hip_grid  test_compare_mismatch
                     k_level<true>                    gt4hip_grid  LEFT OUT, for the reason of k_query<true>
  gt4hip_maker.hip   k_mk_summary, k_mk_codes, k_mk_emit<WRITE>
                                                      gt4hip_grid  test_text_to_words, test_text_to_list
                     k_mk_events<WRITE>, k_mk_emit_loc + the three above
                                                      gt4hip_grid  test_text_to_locations, test_text_to_locations_of_a_piece_without_events
                     k_pack_locations                 gt4hip_grid  test_pack_locations
  gt4hip_gmer.hip    k_gmer_prepare, k_gmer_pack      gt4hip_grid  test_gmer_db_create
                     k_gmer_count<AGG>                gt4hip_grid  test_gmer_count_words
                     k_mk_text_counts<FASTQ>          gt4hip_grid  test_gmer_count_text
  gt4hip_subset.hip  k_subset_pass<W, EMIT>           gt4hip_grid  test_subset_seven_tiles
                     k_subset_scan_reduce / _apply, k_subset_compact
                                                      gt4hip_grid  test_subset_scans_of_seven_tiles
                     k_subset_guess, k_subset_changed gt4hip_grid  test_subset_seven_blocks_of_tiles
  gt4hip_select.hip  k_select_decide, k_select_emit   gt4hip_grid  test_table_select
  gt4hip_pairwise.hip k_pairwise_partial              gt4hip_grid  test_table_pairwise
  gt4hip_sort.hip    k_radix_hist                     gt4hip_grid  test_sort_words
  gt4hip_caller.hip  k_caller_probs<ALL>              gt4hip_grid  test_caller_probabilities
                     k_caller_mlogl                   mlogl_grid   NOT capped: the grid decides the bits of the sum.
                                                                   tests/test_caller_gpu.py runs it above 256 and at 1024
                                                                   workgroups and shows that "grid_cap" leaves it alone
  gt4hip_kernels.hip k_generate                       grid_for     test_generate
                     k_sum_counts, k_check_sorted     grid_for     test_sum_counts_and_is_sorted
                     k_decode_index                   grid_for     test_upload_index
                     k_extract_keys, k_extract_column grid_for     test_count_table_by_merges
                     k_partition                      NOT capped: one thread per tile boundary by construction (the loop
                                                                   only deals the words it zeroes); a partition kernel
                     k_pair_merge (n_workers)         NOT capped: its workgroups wait for one another; option "grid",
                                                                   under which tests/test_few_workers_gpu.py runs it with
                                                                   one to three workgroups
  gt4hip_multi.hip   k_sample_stride                  gt4hip_grid  test_shard_cuts
  gt4hip_nway_part.h k_nway_sample                    NOT capped: a partition kernel of the N-way family, which keeps "grid"
  gt4hip_nway_tile.h k_nway_merge (n_workers)         NOT capped: its workgroups wait for one another; option "grid",
                                                                   under which tests/test_few_workers_gpu.py runs it with
                                                                   one to four workgroups
"""
import numpy as np
import pytest

import gpu_util
import maker_model as MK
import gmer_model as GM
import mismatch_model as MM
import pairwise_model as PM
import query_model as QM
import select_model as SEL
import select_util as SU
import subset_model as SM
from genometester4_amd import capi
from genometester4_amd.listio import make_records
from test_caller_gpu import PAIRS, _capi_model, check_probabilities
from test_gindex_gpu import back, model_of, on_device
from test_gmaker_gpu import bases
from test_gmer_gpu import _canonical, _db_words, _expect, _queries
from test_gqloc_gpu import Synth, canon_words
from test_hit_pass_gpu import expect_exact
from test_pairwise_gpu import make_lists as pairwise_lists
from test_select_gpu import make_lists as select_lists
from test_subset_gpu import _counts_with_sum

pytestmark = pytest.mark.gpu

CAPS = (1, 2, 3)
BLOCKS = 7
FULL = pytest.mark.parametrize("full", [False, True], ids=["6+1", "7"])
CAP = pytest.mark.parametrize("cap", CAPS)


@pytest.fixture(scope="module")
def ctx():
    """a context of this module's own: no other file sees a cap.  "poison": the capped run gets its device blocks from the
    pool, where the uncapped run has just left the right results; an item that a broken stride skips must not keep them"""
    c = capi.Context(0)
    c.set_option("poison", 1)
    yield c
    c.set_option("grid_cap", 0)
    c.close()


def size(block, full):
    """items of seven blocks of `block` items: six full ones and one item, or seven full ones"""
    return BLOCKS * block if full else (BLOCKS - 1) * block + 1


def blocks(items, block):
    return (items + block - 1) // block


def frozen(x):
    """a result as something == compares byte for byte"""
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    if isinstance(x, (tuple, list)):
        return tuple(frozen(v) for v in x)
    if isinstance(x, dict):
        return tuple((k, frozen(v)) for k, v in sorted(x.items()))
    return x


def capped(ctx, cap, launches, call, uncut=True):
    """call () uncapped, then under "grid_cap" = cap: the counter, the two results byte for byte; returns the capped one.
    uncut = False: a kernel of the call has more blocks of work than the built-in cap as well"""
    before = ctx.get_counter("grid_capped")
    plain = call()
    middle = ctx.get_counter("grid_capped")
    assert middle == before or not uncut, "the uncapped run was cut: its input is too large for this test"
    ctx.set_option("grid_cap", cap)
    try:
        got = call()
    finally:
        ctx.set_option("grid_cap", 0)
    cut = ctx.get_counter("grid_capped") - middle
    assert cut >= launches, "%d launches were cut, the call has %d that stride" % (cut, launches)
    assert frozen(got) == frozen(plain), "the capped run differs from the uncapped one"
    return got


_once = {}


def once(key, make):
    """a model's answer or an input, made once and left as it is"""
    if key not in _once:
        _once[key] = make()
    return _once[key]


# ------------------------------------------------------------------ glistquery

@pytest.fixture(scope="module")
def W(ctx):
    """items per block of the item loops (MM_THREADS)"""
    return ctx.get_counter("mm_threads")


@pytest.fixture(scope="module")
def T(ctx, W):
    """items per tile of the hit and compaction passes (MM_TILE)"""
    t = ctx.get_counter("mm_tile")
    assert t % W == 0 and t > W
    return t


def distinct_keys(rng, n, bits=50):
    """n different keys below 2^bits, ascending"""
    keys = np.unique(rng.integers(0, 1 << bits, size=n + n // 4 + 8, dtype=np.uint64))
    keys = np.sort(rng.permutation(keys)[:n])
    assert len(keys) == n
    return keys


def query_list(k, n_keys, seed):
    """canonical words, a count each (zeros and all-ones among them)"""
    def make():
        rng = np.random.default_rng(seed)
        space = 1 << (2 * k)
        keys = np.unique(QM.canonical_np(rng.integers(0, space, size=3 * n_keys, dtype=np.uint64), k))
        keys = np.sort(rng.permutation(keys)[:n_keys])
        counts = rng.integers(1, 200, size=len(keys), dtype=np.uint32)
        counts[::97] = 0
        counts[1::97] = 0xFFFFFFFF
        return keys, counts
    return once(("query_list", k, n_keys, seed), make)


def query_words(keys, k, n, seed, rate=0.5):
    """n words, about `rate` of them words of the list on either strand"""
    rng = np.random.default_rng(seed)
    words = rng.integers(0, 1 << (2 * k), size=n, dtype=np.uint64)
    take = rng.random(n) < rate
    words[take] = keys[rng.integers(0, len(keys), size=int(take.sum()))]
    flip = rng.random(n) < 0.5
    words[flip] = QM.revcomp_np(words[flip], k)
    return words


@CAP
@FULL
def test_lookup_exact(ctx, W, cap, full):
    """k_query_exact: one launch"""
    k = 25
    keys, counts = query_list(k, 3000, 1)
    words = query_words(keys, k, size(W, full), 2)
    words[[0, -1]] = keys[[5, 6]]  # the first item and the last one of the last trip hit
    ix = ctx.upload(make_records(keys, counts), k).query_index()
    val, found = capped(ctx, cap, 1, lambda: ix.lookup(words))
    ix.free()
    ev, ef = QM.lookup_np(keys, counts, words, k)
    assert ef.sum() > len(words) // 3 and ef[0] and ef[-1]
    assert (val == ev).all() and (found == ef).all()


# k = 9: 28 variants with one mismatch, 352 with two, 277 with two outside the last base: none divides the 256 threads of a
# workgroup, so a query's variants straddle workgroups and trips.  64 x 28 = 7 x 256; no number of variants of two
# mismatches divides 7 x 256 (16 at k = 2 does, and divides 256), so those cases have a partial last block only.
MISMATCH_SHAPES = {"mm1-6+1": (1, 0, 55), "mm1-7": (1, 0, 64), "mm2-6+224": (2, 0, 5), "mm2-6+126": (2, 1, 6), "found-6+1": (1, 0, None), "found-7": (1, 0, None)}


@CAP
@pytest.mark.parametrize("shape", list(MISMATCH_SHAPES))
def test_lookup_with_mismatches(ctx, W, cap, shape):
    """k_query (its stride carry r += stride_r, w += stride_w comes from the grid) and k_query_found: "found-*" have seven
    blocks of queries for k_query_found (and 169 or 196 blocks of variants), the others seven blocks of variants"""
    k = 9
    n_mm, pm_3, n = MISMATCH_SHAPES[shape]
    n_var = capi.query_variants(k, n_mm, pm_3)
    assert W % n_var
    if n is None:
        n = size(W, shape == "found-7")
        launches = 2
    else:
        assert blocks(n * n_var, W) == BLOCKS and (n * n_var > (BLOCKS - 1) * W)
        assert shape != "mm1-7" or n * n_var == BLOCKS * W
        launches = 1
    keys, counts = query_list(k, 40_000, 3)  # a third of the canonical 9-mers: variants do hit
    words = query_words(keys, k, n, 4 + n)
    ix = ctx.upload(make_records(keys, counts), k).query_index()
    val, found = capped(ctx, cap, launches, lambda: ix.lookup(words, n_mm, pm_3))
    ix.free()
    ev, ef = once(("mm", shape), lambda: QM.lookup_np(keys, counts, words, k, n_mm, pm_3))
    assert ef.sum() > n // 2
    assert (val == ev).all() and (found == ef).all()


def expected_hits(keys, counts, words, k, n_mm, pm_3):
    """every variant found, in (query, rank) order: the masks by rank from the library's host function, the rest numpy"""
    q = QM.canonical_np(np.asarray(words, dtype=np.uint64), k)
    n_var = capi.query_variants(k, n_mm, pm_3)
    rows = []
    for r in range(n_var):
        v = QM.canonical_np(q ^ np.uint64(capi.query_variant_mask(k, n_mm, pm_3, r)), k)
        present, cnt = QM.find_np(keys, counts, v)
        at = np.flatnonzero(present)
        h = np.zeros(len(at), dtype=capi.QUERY_HIT_DTYPE)
        h["query"], h["rank"], h["word"], h["count"] = at, r, v[at], cnt[at]
        rows.append(h)
    out = np.concatenate(rows)
    return out[np.lexsort((out["rank"], out["query"]))]


@CAP
@pytest.mark.parametrize("shape", ["mm0-6+1", "mm0-7", "mm1-6+4", "mm1-7"])
def test_lookup_all(ctx, T, cap, shape):
    """k_query_hits<FILL, false>: the count pass and the fill pass over seven tiles, two launches"""
    if shape.startswith("mm0"):
        k, n_mm, n = 25, 0, size(T, shape == "mm0-7")
        keys, counts = query_list(k, 3000, 1)
    else:
        k, n_mm = 9, 1
        n_var = capi.query_variants(k, 1, 0)
        n = BLOCKS * T // n_var if shape == "mm1-7" else ((BLOCKS - 1) * T) // n_var + 1
        assert blocks(n * n_var, T) == BLOCKS and (shape != "mm1-7" or n * n_var == BLOCKS * T)
        keys, counts = query_list(k, 40_000, 3)
    words = query_words(keys, k, n, 5 + n)
    words[[0, -1]] = keys[[5, 6]]
    want = once(("all", shape), lambda: expected_hits(keys, counts, words, k, n_mm, 0))
    ix = ctx.upload(make_records(keys, counts), k).query_index()
    hits = capped(ctx, cap, 2, lambda: ix.lookup_all(words, n_mm, 0, capacity=len(want) + 1))
    ix.free()
    assert len(want) > n // 3
    assert len(hits) == len(want) and (hits == want).all()


@CAP
@FULL
def test_index_build(ctx, W, cap, full):
    """k_index_build strides over the n records and the slot behind them: n + 1 items in seven blocks.  The index is read
    through exact lookups of every word of the list and as many absent ones (k_query_exact: 14 blocks)"""
    k = 25
    n = size(W, full) - 1
    keys, counts = query_list(k, n, 6 + n)
    assert len(keys) == n and blocks(n + 1, W) == BLOCKS
    counts = np.where(counts == 0, 7, counts).astype(np.uint32)
    absent = np.setdiff1d(query_list(k, n, 7 + n)[0], keys)
    words = np.concatenate([keys, absent])
    lst = ctx.upload(make_records(keys, counts), k)

    def call():
        ix = lst.query_index()
        out = ix.lookup(words)
        ix.free()
        return out

    val, found = capped(ctx, cap, 2, call)
    assert found[:n].all() and (val[:n] == counts).all() and not found[n:].any() and not val[n:].any()


def location_index(ctx, W, full):
    """an index of seven blocks of words for k_index_split, most with one location, empty and long segments among them"""
    n = size(W, full)
    w = canon_words(12, n, 30 + n)
    assert len(w) == n
    rng = np.random.default_rng(n)
    counts = np.ones(n, dtype=np.uint64)
    counts[rng.integers(0, n, size=40)] = 0
    counts[[0, 9, n - 1]] = [0, 3 * ctx.get_counter("gather_tile") + 5, 4]
    return w, counts


@pytest.fixture(scope="module")
def synths(ctx, W):
    """the two indexes of location_index, resident for the module and freed before its context closes"""
    made = {full: Synth(ctx, 12, *location_index(ctx, W, full)) for full in (False, True)}
    yield made
    for s in made.values():
        s.dev.free()


@CAP
@FULL
def test_location_index_create(ctx, W, synths, cap, full):
    """k_index_split over seven blocks of k-mer entries, then k_index_build; read through a lookup of every word"""
    w, counts = location_index(ctx, W, full)

    def call():
        s = Synth(ctx, 12, w, counts)
        out = s.dev.lookup(w)
        s.dev.free()
        return out

    hits, locs = capped(ctx, cap, 2, call)
    eh, el = expect_exact(synths[full], w)  # (the numpy side of the same index)
    assert len(hits) == len(w) and (hits == eh).all() and len(locs) == int(counts.sum()) and (locs == el).all()


@CAP
@FULL
def test_location_lookup(ctx, W, T, synths, cap, full):
    """gt4hip_query_lookup_locations, size then fill: the count pass (twice), the fill pass and the gather, four launches.
    Seven tiles of queries AND seven tiles of locations: one hit with a segment of three gather tiles and five, unit
    segments and empty ones for the rest of the locations, absent words for the rest of the queries"""
    G = ctx.get_counter("gather_tile")
    w, counts = location_index(ctx, W, True)
    s = synths[True]
    rng = np.random.default_rng(77 + full)
    n, n_loc = size(T, full), size(G, full)
    unit, empty = np.flatnonzero(counts == 1), np.flatnonzero(counts == 0)
    hit_words = np.concatenate([w[[9]], w[rng.choice(unit, size=n_loc - int(counts[9]) - 2)], w[empty[:20]]])
    absent = np.setdiff1d(canon_words(12, 3000, 5), w)
    q = absent[rng.integers(0, len(absent), size=n)]
    q[1 + np.sort(rng.choice(n - 2, size=len(hit_words), replace=False))] = rng.permutation(hit_words)
    q[[0, n - 1]] = w[unit[:2]]  # the first and the last query hit
    eh, el = once(("loc", full), lambda: expect_exact(s, q))
    assert len(eh) == len(hit_words) + 2 and len(el) == n_loc and blocks(len(el), G) == BLOCKS
    hits, locs = capped(ctx, cap, 4, lambda: s.dev.lookup(q))
    assert len(hits) == len(eh) and (hits == eh).all()
    assert len(locs) == len(el) and (locs == el).all()


@CAP
@FULL
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "slice1"])
def test_list_statistics(ctx, W, cap, full, aligned):
    """for_each_record under k_count_stats, k_count_split, k_count_histogram (bins in LDS, bins in global memory) and k_gc:
    four records a thread from a 16-byte aligned list, one a thread from slice (1, n) of it; five launches"""
    k, n = 25, size(4 * W, full)
    bins = ctx.get_counter("hist_lds_bins")
    rng = np.random.default_rng(n)
    keys = distinct_keys(rng, n + 1)
    c = rng.integers(1, 300, size=n + 1, dtype=np.uint32)
    c[rng.integers(0, n + 1, size=200)] = rng.integers(300, bins + 900, size=200)
    c[[1, n - 1, n]] = [0, 0xFFFFFFFF, 0xFFFFFFF0]
    whole = ctx.upload(make_records(keys, c), k)
    lst = whole.slice(0, n) if aligned else whole.slice(1, n)
    keys, c = (keys[:n], c[:n]) if aligned else (keys[1:], c[1:])
    assert (lst.device_ptr % 16 == 0) == aligned
    got = capped(ctx, cap, 5, lambda: (lst.count_stats(), lst.count_split(150), lst.count_histogram(300), lst.count_histogram(bins + 904), lst.gc()))
    assert got[0] == (int(c.min()), int(c.max()))
    assert got[1] == (int((c < 150).sum()), int((c > 150).sum()))
    for hist, mx in ((got[2], 300), (got[3], bins + 904)):
        exp = np.bincount(c[(c >= 1) & (c <= mx)], minlength=mx + 1)[1:mx + 1]
        assert (hist == exp.astype(np.uint64)).all(), mx
    assert got[4] == QM.gc_bases(keys, c, k)


# ------------------------------------------------------------------ glistcompare -mm

def mismatch_pair(n, k=9):
    """the first list has n words (seven tiles of the compaction); the second holds 40 % of them and 3000 others (four
    tiles): as tests/test_hit_pass_gpu.py builds its pairs"""
    def make():
        rng = np.random.default_rng(n)
        ka = np.sort(rng.choice(1 << (2 * k), size=n, replace=False)).astype(np.uint64)
        inner = ka[1:-1]
        kb = np.setdiff1d(np.concatenate([inner[rng.random(len(inner)) < 0.4], rng.integers(0, 1 << (2 * k), size=3000, dtype=np.uint64)]), ka[[0, -1]])
        ca = rng.integers(1, 5, size=len(ka), dtype=np.uint32)
        ca[[0, -1]] = 4
        return make_records(ka, ca), make_records(kb, rng.integers(1, 5, size=len(kb), dtype=np.uint32))
    return once(("mm_pair", n), make)


@CAP
@FULL
@pytest.mark.parametrize("subtract", [False, True], ids=["keep", "subtract"])
@pytest.mark.parametrize("n_mm", [1, 2])
def test_compare_mismatch(ctx, T, cap, full, n_mm, subtract):
    """both complements: two index builds, two pre-passes (49 or 56 blocks and about 30), the compaction of each pre-pass
    (k_tile_count and k_scatter over seven tiles and over four): eight launches at least, then the level kernel, k_decide
    and a compaction per level and list.  Level 2 has 324 variants a word: with the thousands of words that seven tiles
    leave, more blocks than the built-in cap, so with two mismatches the uncapped run is cut there as well."""
    k = 9
    a, b = mismatch_pair(size(T, full))
    assert blocks(len(a), T) == BLOCKS and blocks(len(b), T) > max(CAPS)
    exp = once(("mm_model", full, n_mm, subtract), lambda: MM.compare_mismatch(a, b, k, n_mm, 2, subtract, True))
    assert len(exp[4]) < len(a) and len(exp[8]) < len(b) and (n_mm == 2 or (len(exp[4]) > 100 and len(exp[8]) > 100))  # (hardly a 9-mer is without a neighbour at two mismatches)
    da, db = ctx.upload(a, k), ctx.upload(b, k)

    def call():
        st, out, _ = ctx.compare_mismatch(da, db, capi.OP_DIFF1 | capi.OP_DIFF2, n_mm, cutoff=2, subtract=subtract)
        got = {bit: out[bit].download() for bit in out}
        for o in out.values():
            o.free()
        return st, got

    st, got = capped(ctx, cap, 8, call, uncut=n_mm == 1)
    for bit, rec in exp.items():
        assert got[bit].tobytes() == rec.tobytes(), (bit, len(got[bit]), len(rec))
        assert st[bit] == MM.totals(rec)
    da.free()
    db.free()


# ------------------------------------------------------------------ glistmaker

@pytest.fixture(scope="module")
def MT(ctx):
    """bytes of text per tile of the reader's kernels"""
    t = ctx.get_counter("maker_text_tile")
    assert t == ctx.get_counter("maker_code_tile")
    return t


def fasta_text(n_bytes, tile):
    """exactly n_bytes of FastA: lines of 61 bases, so a sequence line and the words in it straddle every tile edge; a name
    line of 200 bytes, with '>' and bases in it, begins in tile 2 and ends in tile 3.  Under "grid_cap" = 1 all those tiles
    are consecutive trips of one workgroup."""
    def make():
        rng = np.random.default_rng(n_bytes)
        out = bytearray(b">s\n")
        named = False
        while len(out) < n_bytes:
            if not named and len(out) >= 3 * tile - 62:
                assert len(out) < 3 * tile
                out += b">" + (b"ACGT>ACGTAC " * 20)[:198] + b"\n"
                named = True
            out += bases(61, rng) + b"\n"
        text = bytes(out[:n_bytes])
        at = text.index(b">ACGT>ACGTAC")
        assert at < 3 * tile < at + 199
        return text
    return once(("fasta", n_bytes), make)


def fastq_text(n_bytes, tile):
    """exactly n_bytes of FastQ, whole records of 101 bases (the last one sized to end the text): records straddle every
    tile edge; the name of one, 300 bytes with '@', '+' and '>' in it, begins in tile 2 and ends in tile 3"""
    def make():
        rng = np.random.default_rng(n_bytes + 1)
        out = bytearray()
        r = 0
        while len(out) < n_bytes - 700:
            name = b"@r%d" % r
            if 3 * tile - 215 <= len(out) < 3 * tile:
                name = b"@" + (b"n>+@ACGT " * 40)[:299]
                assert len(out) + len(name) > 3 * tile
            seq = bytearray(bases(101, rng))
            if r % 9 == 0:
                seq[int(rng.integers(0, 101))] = ord("N")
            out += name + b"\n" + seq + b"\n+\n" + b"I" * 101 + b"\n"
            r += 1
        rest = n_bytes - len(out)
        length, extra = (rest - 7) // 2, (rest - 7) % 2
        out += b"@z" + b"x" * extra + b"\n" + bases(length, rng) + b"\n+\n" + b"I" * length + b"\n"
        assert len(out) == n_bytes
        return bytes(out)
    return once(("fastq", n_bytes), make)


TEXTS = {"fasta": fasta_text, "fastq": fastq_text}


@CAP
@FULL
@pytest.mark.parametrize("kind", list(TEXTS))
def test_text_to_words(ctx, MT, cap, full, kind):
    """k_mk_summary, k_mk_codes, k_mk_emit counting and k_mk_emit writing over seven tiles: four launches"""
    k = 16
    text = TEXTS[kind](size(MT, full), MT)
    assert blocks(len(text), MT) == BLOCKS
    exp, err = once(("words", kind, full, k), lambda: MK.read_words(text, k))
    assert err is None and len(exp) > MT

    def call():
        words, carry = ctx.text_to_words(text, k)
        return words, bytes(carry)

    words, _ = capped(ctx, cap, 4, call)
    assert words.tolist() == exp


@CAP
@FULL
def test_text_to_list(ctx, MT, cap, full):
    """the reader's four launches, then the sort and fold of its words (k_radix_hist strides over them too)"""
    k = 25
    text = fasta_text(size(MT, full), MT)
    keys, counts = once(("list", full, k), lambda: MK.fold(MK.read_words(text, k)[0]))

    def call():
        lst = ctx.text_to_list(text, k)
        rec = lst.download()
        lst.free()
        return rec

    got = capped(ctx, cap, 4, call)
    assert got["key"].tolist() == keys.tolist() and got["count"].tolist() == counts.tolist()


@CAP
@FULL
@pytest.mark.parametrize("kind", list(TEXTS))
def test_text_to_locations(ctx, MT, cap, full, kind):
    """summary, codes, emit counting, k_mk_events counting and writing, k_mk_emit_loc: six launches"""
    k = 11
    text = TEXTS[kind](size(MT, full), MT)
    want = once(("locations", kind, full, k), lambda: model_of(text, k))
    assert len(want[0]) > MT and len(want[2]) >= 2

    def call():
        words, raw, subs, max_pos = ctx.text_to_locations([text], k)
        return words, raw, subs, max_pos

    words, raw, subs, max_pos = capped(ctx, cap, 6, call)
    assert words.tolist() == want[0]
    assert raw.tolist() == want[1]
    assert subs == want[2] and max_pos == want[3]


@CAP
@FULL
def test_text_to_locations_of_a_piece_without_events(ctx, MT, cap, full):
    """a file in two pieces: a name and a line, then seven tiles from inside the same sequence, which hold no event (FastA:
    a '>' and the end of a name line).  k_mk_events is not launched to write then: the second piece has exactly five
    launches that stride (summary, codes, emit counting, events counting, k_mk_emit_loc), and the first, of one tile, none"""
    k = 11
    rng = np.random.default_rng(MT + full)
    head = b">only\n" + bases(61, rng) + b"\n"
    body = b"".join(bases(61, rng) + b"\n" for _ in range(size(MT, full) // 62 + 1))[:size(MT, full)]
    want = once(("no_events", full), lambda: model_of(head + body, k))
    assert len(want[2]) == 1 and blocks(len(body), MT) == BLOCKS
    before = ctx.get_counter("grid_capped")
    words, raw, subs, max_pos = capped(ctx, cap, 5, lambda: ctx.text_to_locations([head, body], k))
    assert ctx.get_counter("grid_capped") - before == 5
    assert words.tolist() == want[0] and raw.tolist() == want[1]
    assert subs == want[2] and max_pos == want[3]


@CAP
@FULL
def test_pack_locations(ctx, cap, full):
    """k_pack_locations: raw locations (ordinal << 33 | position << 1 | strand) to location words, in place; one launch"""
    n = size(ctx.get_counter("pack_threads"), full)
    rng = np.random.default_rng(n)
    file, sb, pb = 2, 9, 20
    ordinal, pos, strand = rng.integers(0, 1 << sb, size=n, dtype=np.uint64), rng.integers(0, 1 << pb, size=n, dtype=np.uint64), rng.integers(0, 2, size=n, dtype=np.uint64)
    raw = (ordinal << np.uint64(33)) | (pos << np.uint64(1)) | strand

    def call():
        d = on_device(raw)
        ctx.pack_locations(d.data_ptr(), n, file, sb, pb)
        return back(d)

    got = capped(ctx, cap, 1, call)
    # file number in front, then the subsequence, the position and the strand (tests/index_model.py: pairs)
    want = (np.uint64(file) << np.uint64(sb + pb + 1)) | (ordinal << np.uint64(pb + 1)) | (pos << np.uint64(1)) | strand
    assert (got == want).all()


# ------------------------------------------------------------------ gmer_counter

@CAP
@FULL
def test_gmer_db_create(ctx, W, cap, full):
    """k_gmer_prepare and k_gmer_pack over seven blocks of k-mers, then k_index_build; read by counting every k-mer once"""
    k, n = 25, size(W, full)
    dbw = once(("gmer_db", n), lambda: _db_words(np.random.default_rng(n), n, k))
    q = _canonical(dbw, k)

    def call():
        db = ctx.gmer_db(dbw, k)
        out = db.count_words(q), db.counts()
        db.free()
        return out

    (hits, gc), counts = capped(ctx, cap, 3, call)
    want, want_hits, want_gc = _expect(dbw, k, q)
    assert (hits, gc) == (want_hits, want_gc) == (n, want_gc) and np.array_equal(counts, want) and (counts == 1).all()


@CAP
@FULL
@pytest.mark.parametrize("plain", [False, True], ids=["aggregated", "plain_atomics"])
def test_gmer_count_words(ctx, W, cap, full, plain):
    """k_gmer_count over seven blocks of words: one launch"""
    k, n = 25, size(W, full)
    rng = np.random.default_rng(1000 + n)
    dbw = once(("gmer_db", 5000), lambda: _db_words(np.random.default_rng(5000), 5000, k))
    q = once(("gmer_q", n), lambda: _queries(rng, dbw, k, n, 0.5))
    q[[0, -1]] = _canonical(dbw[:2], k)
    db = ctx.gmer_db(dbw, k)

    def call():
        db.reset()
        return db.count_words(q, capi.GMER_PLAIN_ATOMICS if plain else 0), db.counts()

    (hits, gc), counts = capped(ctx, cap, 1, call)
    db.free()
    want, want_hits, want_gc = _expect(dbw, k, q)
    assert want_hits > n // 3
    assert (hits, gc) == (want_hits, want_gc) and np.array_equal(counts, want)


@CAP
@FULL
def test_gmer_count_text(ctx, MT, cap, full):
    """the reader's four launches, k_mk_text_counts over the seven tiles, k_gmer_count over the words: six launches"""
    k = 16
    text = fastq_text(size(MT, full), MT)

    def model():
        words = GM.Reader(text, k).words
        mine = sorted(set(words[::7]))[:1500]
        dbm = GM.Database(k, ["n%d" % i for i in range(len(mine))], [1] * len(mine), [[w] for w in mine])
        counts, st, err = GM.count(dbm, [text])
        assert err is None and len(mine) > 1000 and st["n_hits"] >= len(mine) and st["n_n"] > 0
        return np.array(mine, dtype=np.uint64), counts, st

    dbw, counts, st = once(("gmer_text", full), model)
    db = ctx.gmer_db(dbw, k)

    def call():
        db.reset()
        s, carry = db.count_text(text)
        return {f: getattr(s, f) for f in st}, [int(c) for c in db.counts()]

    got = capped(ctx, cap, 6, call)
    db.free()
    assert got == (st, counts)


# ------------------------------------------------------------------ glistcompare --subset

K = 25


def subset_case(ctx, cap, launches, rec, method, n_size, seed):
    x0 = SM.state48(seed)
    want = once(("walk", rec.tobytes(), method, n_size, x0), lambda: SM.serial_walk(rec, method, n_size, x0))
    lst = ctx.upload(rec, K)

    def call():
        n_words, total, out = ctx.subset(lst, method, n_size, x0)
        got = out.download()
        out.free()
        return n_words, total, got

    n_words, total, got = capped(ctx, cap, launches, call)
    assert got.tobytes() == want.tobytes(), (method, len(rec), n_size)
    assert (n_words, total) == (len(want), int(want["count"].astype(np.uint64).sum()))
    assert lst.download().tobytes() == rec.tobytes()
    lst.free()


@CAP
@FULL
@pytest.mark.parametrize("method", [SM.RAND, SM.RAND_UNIQUE, SM.RAND_WEIGHTED_UNIQUE], ids=["rand", "rand_unique", "rand_weighted_unique"])
def test_subset_seven_tiles(ctx, cap, full, method):
    """k_subset_pass over seven tiles of items, once per pass and once more to write: two launches at least"""
    items = size(ctx.get_counter("subset_tile"), full)
    if method == SM.RAND:  # items are occurrences: counts that add up to them
        n = 1 + items // 3
        rec = SM.make_list(70 + full, n, K, 1)
        rec["count"] = _counts_with_sum(np.random.default_rng(items), n, items)
        subset_case(ctx, cap, 2, rec, method, items // 2, 11)
    else:
        rec = SM.make_list(72 + full, items, K, 30)
        subset_case(ctx, cap, 2, rec, method, items // 2 if method == SM.RAND_UNIQUE else items // 40, 7)


@CAP
@FULL
def test_subset_scans_of_seven_tiles(ctx, cap, full):
    """rand on a list of seven scan tiles of records: k_subset_scan_reduce and _apply over the counts (the item -> record
    map) and over the selected flags, k_subset_compact over the records, k_subset_pass: seven launches at least"""
    n = size(ctx.get_counter("subset_scan_tile"), full)
    rec = SM.make_list(74 + full, n, K, 3)
    rec["count"][5] = 0
    subset_case(ctx, cap, 7, rec, SM.RAND, int(rec["count"].sum()) // 3, 5)


@CAP
@FULL
def test_subset_seven_blocks_of_tiles(ctx, cap, full):
    """k_subset_guess and k_subset_changed take a thread per tile: seven blocks of 256 tiles.  The serial walk of so many
    items takes the model minutes, so SIZE is all of them, as tests/test_subset_gpu.py does at this scale: every item is
    selected and the list comes back less its record without occurrences.  Guess, pass, scans, changed, pass: five at least"""
    tile = ctx.get_counter("subset_tile")
    tiles = size(256, full)
    rec = SM.make_list(76 + full, tiles, K, 1)
    rec["count"] = tile
    rec["count"][[3, tiles - 1]] = [0, 2 * tile]
    items = int(rec["count"].astype(np.uint64).sum())
    assert items == tiles * tile
    lst = ctx.upload(rec, K)

    def call():
        n_words, total, out = ctx.subset(lst, SM.RAND, items, SM.state48(17))
        got = out.download()
        out.free()
        return n_words, total, got, ctx.get_counter("subset_passes")

    n_words, total, got, passes = capped(ctx, cap, 5, call)
    assert got.tobytes() == rec[rec["count"] > 0].tobytes() and (n_words, total) == (tiles - 1, items)
    assert 1 <= passes <= tiles + 1
    lst.free()


# ------------------------------------------------------------------ glistcompare --min_lists / --max_lists, --pairwise

def compact_table(ctx, lists):
    dev = [ctx.upload(l, K) for l in lists]
    table = ctx.device_table(dev)
    table.compact()
    assert not table.ragged
    return dev, table


@CAP
@FULL
@pytest.mark.parametrize("vec", [0, -1], ids=["vec16", "dword"])
def test_table_select(ctx, cap, full, vec):
    """k_select_decide and k_select_emit over the seven segments of a contiguous table of four lists, whose rows are read 16
    bytes a lane or a dword a lane: two launches"""
    seg = ctx.get_counter("select_segment")
    assert seg == SU.select_segment()
    rows, n = size(seg, full), 4
    lists = select_lists(n, rows)
    dev, table = compact_table(ctx, lists)
    assert table.n_keys == rows
    ctx.set_option("select_vec", vec)
    try:
        for m, x, cutoff, rule, ovr in [(1, n, 1, capi.RULE_ADD, 1), (2, 3, 3, capi.RULE_MAX, 1)]:
            rc_w, n_w, t_w, rec_w = once(("select", full, m, x, cutoff, rule), lambda: SEL.select(lists, m, x, cutoff, rule, ovr))
            assert rc_w == 0 and 0 < n_w

            def call():
                rc, cnt, tot, out = ctx.table_select(table, m, x, cutoff, rule, ovr)
                got = out.download()
                out.free()
                return rc, cnt, tot, got, ctx.get_counter("select_wide")

            rc, cnt, tot, got, wide = capped(ctx, cap, 2, call)
            assert wide == (vec == 0)
            assert (rc, cnt, tot) == (0, n_w, t_w) and got.tobytes() == rec_w.tobytes(), (m, x, cutoff, rule)
    finally:
        ctx.set_option("select_vec", 0)
    table.free()
    for d in dev:
        d.free()


@CAP
@FULL
@pytest.mark.parametrize("n", [4, 33])
def test_table_pairwise(ctx, cap, full, n):
    """k_pairwise_partial over seven segments: one launch for four lists, three for 33 (two blocks of list columns, the
    pairs of blocks sharing one grid)"""
    rows = size(ctx.get_counter("select_segment"), full)
    lists, want = pairwise_lists(n, rows)
    dev, table = compact_table(ctx, lists)
    shared, min_total = capped(ctx, cap, 1 if n <= 32 else 3, lambda: ctx.table_pairwise(table))
    assert np.array_equal(shared, want[0]) and np.array_equal(min_total, want[1])
    table.free()
    for d in dev:
        d.free()


# ------------------------------------------------------------------ the radix sort's histogram

@CAP
@FULL
@pytest.mark.parametrize("k", [11, 25])
def test_sort_words(ctx, cap, full, k):
    """gt4hip_sort_words: k_radix_hist strides over chunks of words (the scatter kernels take a workgroup per tile and wait
    for one another: never capped); one launch"""
    n = size(ctx.get_counter("sort_hist_chunk"), full)
    words = np.random.default_rng(n + k).integers(0, 1 << (2 * k), size=n, dtype=np.uint64)

    def call():
        w = on_device(words)
        ctx.sort_words(w.data_ptr(), n, k)
        return back(w)

    got = capped(ctx, cap, 1, call)
    assert (got == np.sort(words)).all()


# ------------------------------------------------------------------ gmer_caller

@CAP
@FULL
@pytest.mark.parametrize("name", ["diploid_lambda30", "size_nonpositive_at_2_lambda"])
def test_caller_probabilities(ctx, cap, full, name):
    """k_caller_probs<true> and <false> over seven blocks of markers: a launch each"""
    n = size(ctx.get_counter("caller_threads"), full)
    pairs = [PAIRS[i % len(PAIRS)] for i in range(n)]
    s = ctx.caller_set([p[0] for p in pairs], [p[1] for p in pairs])
    cm = _capi_model(name)
    all15, plain = capped(ctx, cap, 2, lambda: (s.probabilities(cm, all15=True), s.probabilities(cm)[:3]))
    s.free()
    assert frozen(all15[:3]) == frozen(plain)
    check_probabilities(name, pairs, *all15)


# ------------------------------------------------------------------ the list utilities

@pytest.fixture(scope="module")
def L(ctx):
    """records per block of the list utilities"""
    return ctx.get_counter("list_threads")


@CAP
@FULL
def test_generate(ctx, L, cap, full):
    n = size(L, full)

    def call():
        lst = ctx.alloc(n, 25)
        ctx.generate_ex(lst, n, 11, 29, max_count=9, mult=3, add=1)
        rec = lst.download()
        lst.free()
        return rec

    got = capped(ctx, cap, 1, call)
    assert got.tobytes() == gpu_util.generate_cpu(n, 11, 25, max_count=9, count_seed=29, mult=3, add=1).tobytes()


@CAP
@FULL
def test_sum_counts_and_is_sorted(ctx, L, cap, full):
    """k_sum_counts; k_check_sorted on a sorted list and on lists whose one unsorted pair (i, i + 1) lies across a trip
    boundary of the capped run -- i the last record of the first trip of the last workgroup, i + 1 the first record of the
    second trip of the first -- and across the last one; four launches"""
    n = size(L, full)
    rng = np.random.default_rng(n)
    keys = distinct_keys(rng, n)
    counts = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    lists = [ctx.upload(make_records(keys, counts), 25)]
    for i in (cap * L - 1, n - 2):
        bad = keys.copy()
        bad[[i, i + 1]] = bad[[i + 1, i]]
        assert (np.diff(bad.astype(object)) <= 0).sum() == 1
        lists.append(ctx.upload(make_records(bad, counts), 25))
    got = capped(ctx, cap, 4, lambda: (lists[0].sum_counts(), [l.is_sorted() for l in lists]))
    assert got == (int(counts.astype(np.uint64).sum()), [True, False, False])
    for l in lists:
        l.free()


@CAP
@FULL
def test_upload_index(ctx, L, cap, full):
    """k_decode_index: (word, first location) entries to records whose count is the distance to the next entry's first
    location, the last one's to num_locations, in 32 bits; one launch"""
    n = size(L, full)
    rng = np.random.default_rng(n)
    words = distinct_keys(rng, n)
    per = rng.integers(0, 50, size=n).astype(np.uint64)
    per[n // 2] = (1 << 32) + 5  # truncated to 5
    first = np.concatenate([[0], np.cumsum(per)]).astype(np.uint64)

    def call():
        lst = ctx.upload_index(np.stack([words, first[:-1]], axis=1), int(first[-1]), 25)
        rec = lst.download()
        lst.free()
        return rec

    got = capped(ctx, cap, 1, call)
    assert got.tobytes() == make_records(words, (per & np.uint64(0xFFFFFFFF)).astype(np.uint32)).tobytes()


@CAP
@FULL
def test_count_table_by_merges(ctx, L, cap, full):
    """gt4hip_union_table without the N-way tile kernel (option "kway" = 0): k_extract_keys over the union's seven blocks of
    rows, then k_extract_column per list; three launches"""
    rows = size(L, full)
    lists = select_lists(2, rows)
    dev = [ctx.upload(l, K) for l in lists]
    ctx.set_option("kway", 0)
    try:
        keys, counts = capped(ctx, cap, 3, lambda: ctx.union_table(dev))
        assert not ctx.last_table_was_ragged
    finally:
        ctx.set_option("kway", 1)
    want_keys, want_counts = PM.count_table(lists)
    assert len(keys) == rows and np.array_equal(keys, want_keys) and np.array_equal(counts, want_counts)
    for d in dev:
        d.free()


@CAP
@FULL
def test_shard_cuts(ctx, L, cap, full):
    """gt4hip_shard_cuts: k_sample_stride takes every key of two short lists (stride 1), seven blocks each; two launches.
    First key of shard g: one above the sample at g / n_shards of all samples in order, never below the shard before"""
    n, n_shards = size(L, full), 5
    rng = np.random.default_rng(n)
    keys = [distinct_keys(rng, n, 40) for _ in range(2)]
    dev = [ctx.upload(make_records(k, np.ones(n, dtype=np.uint32)), 25) for k in keys]
    got = capped(ctx, cap, 2, lambda: ctx.shard_cuts(dev, n_shards))
    samples = np.sort(np.concatenate(keys))
    want = [0]
    for g in range(1, n_shards):
        want.append(max(int(samples[len(samples) * g // n_shards - 1]) + 1, want[-1]))
    assert got == want
    for d in dev:
        d.free()
