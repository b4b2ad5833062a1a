"""gt4hip_location_index_create / gt4hip_query_lookup_locations on the device, on SYNTHETIC indexes made in numpy and
checked against an enumeration in Python, at the smallest shapes where the segmented gather can go wrong (T = its output
tile): a segment of 3 T + 5 between unit segments, segments that end and start exactly at a tile edge, a tile of unit
segments only, empty segments (also more of them than a tile keeps in LDS), the last word (whose count comes from
num_locations), one hit, no hit, bit sizes with no file bits and with all 64 bits used, k-mer sections that must be
refused, capacities one too small, and two variants of a query with the same canonical word.  Then the command line:
every transcript of tests/golden/gqloc_cases.json byte for byte, the two large ones on indexes made by our own
glistmaker --index, and a run whose batches are cut in halves by a tiny location budget."""
import os
import re
import shutil

import numpy as np
import pytest

import gqloc_util as U
import query_model as M
from genometester4_amd import capi

pytestmark = pytest.mark.gpu
EFORMAT = 11
SRC = open(os.path.join(U.ROOT, "genometester4_amd", "csrc", "gt4hip_query.hip")).read()
HDR = open(os.path.join(U.ROOT, "genometester4_amd", "csrc", "gt4hip_index.h")).read()
assert re.search(r"GATHER_TILE = MM_THREADS \* GATHER_ROUNDS;", SRC)  # the tile is what the two constants make it
T = int(re.search(r"MM_THREADS = (\d+);", HDR).group(1)) * int(re.search(r"GATHER_ROUNDS = (\d+);", SRC).group(1))  # output locations per tile


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


class Synth:
    """an index in numpy: canonical words ascending, a count each, random packed locations"""

    def __init__(self, ctx, k, words, counts, bits=(2, 10, 20), seed=1, top_bit=False):
        self.k, self.bits = k, bits
        self.words = np.asarray(words, dtype=np.uint64)
        assert (np.diff(self.words.astype(object)) > 0).all()
        self.counts = np.asarray(counts, dtype=np.uint64)
        self.first = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.uint64)
        rng = np.random.default_rng(seed)
        n = int(self.first[-1])
        used = sum(bits) + 1
        self.locs = rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=n, dtype=np.uint64)
        if used < 64:
            self.locs &= np.uint64((1 << used) - 1)
        if top_bit and n:
            self.locs[::2] |= np.uint64(1 << 63)
        self.dev = capi.LocationIndex(ctx, np.stack([self.words, self.first[:-1]], axis=1), self.locs, k, bits)
        self.where = {int(w): i for i, w in enumerate(self.words.tolist())}

    def decode(self, codes):
        fb, sb, pb = self.bits
        c = [int(x) for x in codes]

        def field(x, shift, bits):
            return (x >> shift) & ((1 << bits) - 1) if shift < 64 else 0

        out = np.zeros(len(c), dtype=capi.LOCATION_DTYPE)
        out["pos_dir"] = [(field(x, 1, pb) << 1) | (x & 1) for x in c]
        out["file"] = [field(x, sb + pb + 1, fb) & 0xFFFFFFFF for x in c]
        out["seq"] = [field(x, pb + 1, sb) & 0xFFFFFFFF for x in c]
        return out

    def expect(self, queries, n_mm=0, pm_3=0):
        """hits in (query, rank) order and their locations, by enumeration"""
        k = self.k
        masks = [capi.query_variant_mask(k, n_mm, pm_3, r) for r in range(capi.query_variants(k, n_mm, pm_3))]
        hits, codes = [], []
        for qi, q in enumerate(queries):
            c = M.canonical(int(q), k)
            for r, m in enumerate(masks):
                v = M.canonical(c ^ m, k)
                i = self.where.get(v)
                if i is not None:
                    hits.append((qi, r, v, int(self.counts[i]) & 0xFFFFFFFF, 0))
                    codes.append(self.locs[int(self.first[i]):int(self.first[i + 1])])
        return np.array(hits, dtype=capi.QUERY_HIT_DTYPE), self.decode(np.concatenate(codes) if codes else [])

    def check(self, queries, n_mm=0, pm_3=0):
        eh, el = self.expect(queries, n_mm, pm_3)
        hits, locs = self.dev.lookup(queries, n_mm, pm_3)
        assert len(hits) == len(eh) and (hits == eh).all(), (len(hits), len(eh))
        assert len(locs) == len(el) and int(hits["count"].astype(np.uint64).sum()) == len(locs)
        bad = np.flatnonzero(locs != el)
        assert len(bad) == 0, (len(bad), bad[:5], locs[bad[:3]], el[bad[:3]])
        return hits, locs


def canon_words(k, n, seed):
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 1 << (2 * k), size=3 * n, dtype=np.uint64)
    return np.unique(M.canonical_np(w, k))[:n]


def test_one_long_segment_between_unit_segments(ctx):
    w = canon_words(12, 41, 3)
    counts = np.ones(41, dtype=np.uint64)
    counts[20] = 3 * T + 5
    s = Synth(ctx, 12, w, counts)
    s.check(w)                                        # in index order: the long segment starts at output 20
    s.check(np.concatenate([w[20:21], w[::-1], w[20:21]]))  # ... at 0, in the middle, and at the end of the output
    s.check(w[20:21])                                 # a single hit, tiles inside one segment only
    s.dev.free()


def test_segments_that_end_and_start_at_a_tile_edge(ctx):
    w = canon_words(12, 8, 4)
    s = Synth(ctx, 12, w, [T - 3, 3, 5, 1, T - 6, T, 1, 2 * T])  # ends at T, starts at T; ... at 2 T, 3 T, 3 T + 1
    s.check(w)
    s.check(w[[5, 7, 0, 1]])                          # T, then 2 T, then T - 3 + 3: every boundary on an edge
    s.dev.free()


def test_a_tile_of_unit_segments_only(ctx):
    w = canon_words(12, 3 * T + 7, 5)
    s = Synth(ctx, 12, w, np.ones(len(w), dtype=np.uint64), bits=(0, 12, 30))  # no file bits
    hits, locs = s.check(w[::-1])
    assert (hits["count"] == 1).all() and (locs["file"] == 0).all() and len(locs) == 3 * T + 7
    s.dev.free()


def test_empty_segments_and_the_last_word(ctx):
    w = canon_words(12, 2 * T + 900, 6)
    counts = np.ones(len(w), dtype=np.uint64)
    counts[5] = 0                                     # two equal first locations
    counts[T + 10:T + 10 + T + 300] = 0               # more empty segments in a row than a tile keeps in LDS
    counts[-1] = 7                                    # the last word: its count comes from num_locations
    s = Synth(ctx, 12, w, counts)
    hits, locs = s.check(w)
    assert (hits["count"] == 0).sum() == T + 301 and hits["count"][-1] == 7
    s.check(w[[5, len(w) - 1, 5, 5]])                 # empty segments first and last
    h, l = s.check(w[5:6])                            # a hit without a location
    assert len(h) == 1 and len(l) == 0
    s.dev.free()


def test_no_hit_and_capacities_one_too_small(ctx):
    w = canon_words(12, 300, 7)
    counts = np.random.default_rng(7).integers(1, 40, size=300).astype(np.uint64)
    s = Synth(ctx, 12, w, counts)
    absent = np.setdiff1d(canon_words(12, 400, 8), w)[:50]
    nh, nl, hits, locs = s.dev.lookup_raw(absent, hit_capacity=4, loc_capacity=4)
    assert (nh, nl) == (0, 0) and (hits.view(np.uint8) == 0xA5).all() and (locs.view(np.uint8) == 0xA5).all()  # nothing written
    eh, el = s.expect(w)
    for hc, lc in ((len(eh) - 1, len(el)), (len(eh), len(el) - 1), (0, 0)):
        nh, nl, hits, locs = s.dev.lookup_raw(w, hit_capacity=hc, loc_capacity=lc)
        assert (nh, nl) == (len(eh), len(el))         # both totals all the same
        assert (hits.view(np.uint8) == 0xA5).all() and (locs.view(np.uint8) == 0xA5).all()
    nh, nl, hits, locs = s.dev.lookup_raw(w, hit_capacity=len(eh), loc_capacity=len(el))
    assert (hits == eh).all() and (locs == el).all()
    s.dev.free()


@pytest.mark.parametrize("bits", [(0, 31, 32), (1, 30, 32), (0, 0, 63), (20, 20, 23)], ids=str)
def test_bit_sizes_up_to_all_64_bits(ctx, bits):
    w = canon_words(16, 500, 9)
    counts = np.random.default_rng(9).integers(0, 9, size=500).astype(np.uint64)
    s = Synth(ctx, 16, w, counts, bits=bits, top_bit=True)
    _, locs = s.check(w)
    assert sum(bits) + 1 < 64 or (s.locs >> np.uint64(63)).any()
    s.dev.free()
    with pytest.raises(capi.Gt4HipError) as e:        # 65 bits
        capi.LocationIndex(ctx, np.zeros((1, 2), dtype=np.uint64), np.zeros(1, dtype=np.uint64), 16, (bits[0] + 1, bits[1], bits[2]) if sum(bits) == 63 else (1, 31, 32))
    assert e.value.code == EFORMAT


def test_a_kmer_section_that_points_outside_is_refused(ctx):
    w = canon_words(12, 5000, 10)
    first = np.arange(5000, dtype=np.uint64) * np.uint64(2)
    locs = np.zeros(10000, dtype=np.uint64)
    for at, value in ((2500, 3), (4999, 10001), (0, 1 << 63), (4100, (1 << 64) - 1)):  # descends; above num_locations
        f = first.copy()
        f[at] = value
        with pytest.raises(capi.Gt4HipError) as e:
            capi.LocationIndex(ctx, np.stack([w, f], axis=1), locs, 12, (2, 10, 20))
        assert e.value.code == EFORMAT, (at, value)
    ok = capi.LocationIndex(ctx, np.stack([w, first], axis=1), locs, 12, (2, 10, 20))  # the same arrays unharmed: accepted
    ok.free()


def test_two_variants_with_one_canonical_word_count_twice(ctx):
    k = 2
    ag, at = M.string_to_word("AG", 2), M.string_to_word("AT", 2)
    s = Synth(ctx, k, [M.string_to_word("AC", 2), ag], [3, 5])
    hits, locs = s.check([at], n_mm=1)                # CT and AG are both looked up as AG
    assert (hits["word"] == ag).sum() == 2 and len(locs) >= 10
    s.check([at, ag, at], n_mm=2)
    s.dev.free()


def test_random_index_with_skewed_counts(ctx):
    rng = np.random.default_rng(11)
    w = canon_words(12, 20000, 12)
    counts = rng.geometric(0.5, size=len(w)).astype(np.uint64)
    counts[rng.integers(0, len(w), size=6)] = [T, T + 1, 5 * T + 3, 2 * T - 1, 700, 0]
    s = Synth(ctx, 12, w, counts)
    q = np.concatenate([w[rng.integers(0, len(w), size=3000)], rng.integers(0, 1 << 24, size=1000, dtype=np.uint64)])
    s.check(q)
    s.check(q[:600], n_mm=1, pm_3=4)
    assert s.dev.gather_ms > 0
    s.dev.free()


# ------------------------------------------------------------------ the command line

@pytest.fixture(scope="module")
def workdir():
    d = U.make_workdir(built="cli")
    yield d
    shutil.rmtree(d, ignore_errors=True)


@pytest.mark.parametrize("case", U.CASES["cases"], ids=lambda c: c["id"])
def test_every_golden_replays_on_the_gpu(case, workdir):
    p = U.run(case["argv"], workdir)
    assert p.returncode == case["exit"], p.stderr.decode("latin-1")
    U.check_stdout(case, p.stdout)


def test_a_tiny_location_budget_cuts_batches_in_halves(workdir):
    """GT4_GLISTQUERY_LOCATION_BUDGET (tests only): the same bytes by halves; one query over the budget is out of memory"""
    by = {c["id"]: c for c in U.CASES["cases"]}
    for cid, budget in (("s_reads_fq", 16), ("f_q_rev_fwd_mm1", 5), ("big_s_long_k16", 50), ("l_list_mm0", 4), ("q_polya", 290)):
        p = U.run(by[cid]["argv"], workdir, env=dict(GT4_GLISTQUERY_LOCATION_BUDGET=str(budget)))
        assert p.returncode == by[cid]["exit"], (cid, p.stderr)
        U.check_stdout(by[cid], p.stdout)
    p = U.run(by["q_polya"]["argv"], workdir, env=dict(GT4_GLISTQUERY_LOCATION_BUDGET="289"))
    assert p.returncode == 1 and b"out of memory" in p.stderr and b"290" in p.stderr
