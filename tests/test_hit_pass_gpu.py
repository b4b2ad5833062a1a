"""The stable compaction over tiles of MM_TILE items in rounds of a workgroup's threads, at the edges of its rounds and
tiles: the hit pass of gt4hip_query_lookup_all and gt4hip_query_lookup_locations (k_query_hits on round_place, wave_offset,
tile_total and the scans of gt4hip_index.h) and the same steps as gt4hip_compare_mismatch has them (k_tile_count, k_scatter).
W = threads of a workgroup = items of a round, T = MM_TILE = items of a tile, both read from the header.

The hit pass runs on one synthetic location index (test_gqloc_gpu.Synth: k = 12, skewed counts, zeros among them) with one
item per query (n_mm = 0): hits planted at the first and last item of a round, of a tile and of the batch with every other
query absent, 1024 T + T + 5 queries (more tiles than one pass of either scan takes), a tile in which every lane hits
before one in which none does, and 40 queries with two mismatches.  --all and --locations must return the same hits, equal
to numpy's (np.searchsorted on the canonical words; Synth.expect's enumeration where there are variants), and the
locations must be the enumeration's.

k_scatter is driven through gt4hip_compare_mismatch with first lists of the same seven sizes (k = 9, one mismatch, both
complements, subtract on and off) against tests/mismatch_model.py.  tests/test_mismatch_gpu.py has no list of any of these
sizes at k = 9 (its lists are all of 4^k at k <= 6 and planted pairs of 600 to 3000 at k >= 13), so no case is left out."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mismatch_model as MM
import query_model as M
from genometester4_amd import capi
from genometester4_amd.listio import make_records
from test_gqloc_gpu import Synth, canon_words

pytestmark = pytest.mark.gpu
HDR = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "genometester4_amd", "csrc", "gt4hip_index.h")).read()
W = int(re.search(r"MM_THREADS = (\d+);", HDR).group(1))
assert re.search(r"MM_TILE = \(u64\) MM_THREADS \* MM_ROUNDS;", HDR)
T = W * int(re.search(r"MM_ROUNDS = (\d+);", HDR).group(1))
SIZES = [W - 1, W, W + 1, T - 1, T, T + 1, 2 * T + 1]
K = 12


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def index(ctx):
    """3000 canonical words; counts geometric with zeros, a few long ones, the first and the last word among the zeros' and
    the long ones' neighbours; and canonical words the index does not hold"""
    rng = np.random.default_rng(21)
    pool = canon_words(K, 9000, 22)
    rng.shuffle(pool)
    words, absent = np.sort(pool[:3000]), pool[3000:]
    counts = rng.geometric(0.4, size=len(words)).astype(np.uint64)
    counts[rng.integers(0, len(words), size=200)] = 0
    counts[[0, 7, 1500, len(words) - 1]] = [0, 700, 3 * T + 1, 5]
    s = Synth(ctx, K, words, counts)
    s.absent = absent
    yield s
    s.dev.free()


def decode(s, codes):
    fb, sb, pb = s.bits
    out = np.zeros(len(codes), dtype=capi.LOCATION_DTYPE)
    out["pos_dir"] = (((codes >> np.uint64(1)) & np.uint64((1 << pb) - 1)) << np.uint64(1)) | (codes & np.uint64(1))
    out["file"] = (codes >> np.uint64(sb + pb + 1)) & np.uint64((1 << fb) - 1)
    out["seq"] = (codes >> np.uint64(pb + 1)) & np.uint64((1 << sb) - 1)
    return out


def expect_exact(s, queries):
    """n_mm = 0: the hits in query order and their locations, vectorised"""
    c = M.canonical_np(np.asarray(queries, dtype=np.uint64), s.k)
    at = np.minimum(np.searchsorted(s.words, c), len(s.words) - 1)
    found = s.words[at] == c
    rec = at[found]
    hits = np.zeros(len(rec), dtype=capi.QUERY_HIT_DTYPE)
    hits["query"], hits["word"], hits["count"] = np.flatnonzero(found), c[found], s.counts[rec]
    n = s.counts[rec].astype(np.int64)
    start = np.cumsum(n) - n                           # of every hit's locations in the output
    src = np.repeat(s.first[rec].astype(np.int64) - start, n) + np.arange(int(n.sum()))
    return hits, decode(s, s.locs[src])


def lookup_all(s, queries, n_mm=0, pm_3=0):
    """gt4hip_query_lookup_all through the location index's own query index: size, then fill"""
    w = np.ascontiguousarray(queries, dtype=np.uint64)
    prm, n = capi.QueryParams(n_mm, pm_3, 1), C.c_uint64()
    s.dev.ctx._chk(capi.lib().gt4hip_query_lookup_all(s.dev.ctx.h, s.dev.q, w.ctypes.data, len(w), C.byref(prm), None, 0, C.byref(n)))
    hits = np.zeros(n.value, dtype=capi.QUERY_HIT_DTYPE)
    s.dev.ctx._chk(capi.lib().gt4hip_query_lookup_all(s.dev.ctx.h, s.dev.q, w.ctypes.data, len(w), C.byref(prm), hits.ctypes.data if n.value else None,
                                                       n.value, C.byref(n)))
    assert n.value == len(hits)
    return hits


def check(s, queries, expected, n_mm=0, pm_3=0):
    eh, el = expected
    ha = lookup_all(s, queries, n_mm, pm_3)
    hl, locs = s.dev.lookup(queries, n_mm, pm_3)
    assert len(ha) == len(eh) and (ha == eh).all(), (len(ha), len(eh))
    assert len(hl) == len(eh) and (hl == eh).all(), (len(hl), len(eh))
    assert len(locs) == len(el) and (locs == el).all(), (len(locs), len(el), np.flatnonzero(locs != el)[:5] if len(locs) == len(el) else None)
    return eh


def planted(s, n, at, seed):
    """n absent queries with words of the index at the items `at` (those below n): long ones, the last, the first (no
    location), others"""
    rng = np.random.default_rng(seed)
    q = s.absent[rng.integers(0, len(s.absent), size=n)]
    at = sorted({a for a in at if 0 <= a < n})
    q[at] = s.words[np.resize([7, len(s.words) - 1, 0, 1500, 33, 34, 35], len(at))]
    flip = rng.random(n) < 0.5                          # either strand of a query finds the canonical word
    q[flip] = M.revcomp_np(q[flip], s.k)
    return q, at


@pytest.mark.parametrize("n", SIZES)
def test_hits_at_round_tile_and_batch_edges(index, n):
    q, at = planted(index, n, [0, W - 1, W, T - 1, T, n - 1], n)
    eh = check(index, q, expect_exact(index, q))
    assert eh["query"].tolist() == at                  # what was planted is what numpy found


def test_more_tiles_than_one_pass_of_the_scans(index):
    n = 1024 * T + T + 5
    at = [t * T + i for t in (0, 1023, 1024, 1025) for i in (0, 4, W - 1, W, T - 1)]
    q, at = planted(index, n, at, 5)
    eh = check(index, q, expect_exact(index, q))
    assert eh["query"].tolist() == at and at[-1] == n - 1 and {a // T for a in at} == {0, 1023, 1024, 1025}


def test_a_tile_where_every_lane_hits_then_one_where_none_does(index):
    rng = np.random.default_rng(6)
    q = np.concatenate([index.words[rng.integers(0, len(index.words), size=T)], index.absent[:T]])
    eh = check(index, q, expect_exact(index, q))
    assert eh["query"].tolist() == list(range(T))


@pytest.mark.parametrize("pm_3", [0, 3])
def test_two_mismatches(index, pm_3):
    rng = np.random.default_rng(7 + pm_3)
    q = np.concatenate([index.words[rng.integers(0, len(index.words), size=25)], index.absent[:15]])
    eh = check(index, q, index.expect(q, 2, pm_3), 2, pm_3)
    assert (eh["rank"] == 0).sum() == 25 and (eh["rank"] > 0).any()  # the 25 words of the index find themselves; variants hit too


@pytest.mark.parametrize("subtract", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_scatter_at_round_and_tile_edges(ctx, n, subtract):
    """the first list has n words; the second holds 40 % of them, never the first or the last (which the pre-pass keeps
    unless it subtracts), and 1500 others; cutoff 2, so that both complements keep some words and drop some either way"""
    k, rng = 9, np.random.default_rng(n)
    ka = np.sort(rng.choice(1 << (2 * k), size=n, replace=False)).astype(np.uint64)
    inner = ka[1:-1]
    kb = np.setdiff1d(np.concatenate([inner[rng.random(len(inner)) < 0.4], rng.integers(0, 1 << (2 * k), size=1500, dtype=np.uint64)]), ka[[0, -1]])
    ca = rng.integers(1, 5, size=len(ka), dtype=np.uint32)
    ca[[0, -1]] = 4
    a, b = make_records(ka, ca), make_records(kb, rng.integers(1, 5, size=len(kb), dtype=np.uint32))
    d1, d2 = MM.prepass(a, b, 2, subtract, True)
    exp = MM.compare_mismatch(a, b, k, 1, 2, subtract, True)
    assert 0 < len(exp[4]) <= len(d1) < n and 0 < len(exp[8]) <= len(d2) < len(b)  # the pre-pass keeps some and drops some
    assert subtract or (d1["key"][0] == ka[0] and d1["key"][-1] == ka[-1])
    st, out, _ = ctx.compare_mismatch(ctx.upload(a, k), ctx.upload(b, k), capi.OP_DIFF1 | capi.OP_DIFF2, 1, cutoff=2, subtract=subtract)
    for bit, rec in exp.items():
        assert out[bit].download().tobytes() == rec.tobytes(), bit
        assert st[bit] == MM.totals(rec)
