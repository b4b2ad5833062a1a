"""gt4hip_query_lookup / _lookup_all and the list statistics on the device against tests/query_model.py (which
tests/test_gquery_model.py holds to the reference's transcripts), on inputs far larger than the goldens:

  - dense k = 10 (every 10-mer in the list: 4^10 = 1,048,576 records is all there is at that word length) at -mm 0, 1, 2:
    every lane hits, the segmented sum of a wavefront is exercised at every query boundary;
  - iid k = 25, 10^7 records, 10^6 queries with planted 1- and 2-mismatch neighbours, pm_3 0 and 8; -mm 2 runs on all
    10^6 queries and is compared with the model on the planted queries plus a random sample (the numpy model needs
    2,776 passes over the query array at -mm 2);
  - k = 32 with keys 0 and 2^64 - 1 in a list of 10^7 records;
  - batches of 0, 1, 63, 64, 65 and 10^6 + 37 queries (ends inside a wavefront);
  - statistics on 10^8 records with counts up to 2^32 - 1;
  - the binary against oracle/_ref/glistquery on a FastA of ~10^5 25-mers at -mm 1, when that binary is there."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import query_model as M
from genometester4_amd import capi
from genometester4_amd.listio import make_records, write_list

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _check(ix, keys, counts, words, k, n_mm, pm_3, sample=None):
    val, found = ix.lookup(words, n_mm, pm_3)
    sel = np.arange(len(words)) if sample is None else sample
    ev, ef = M.lookup_np(keys, counts, words[sel], k, n_mm, pm_3)
    bad = np.flatnonzero((val[sel] != ev) | (found[sel] != ef))
    assert len(bad) == 0, (k, n_mm, pm_3, len(bad), words[sel][bad[:4]], val[sel][bad[:4]], ev[bad[:4]])
    return val, found


def test_dense_k10(ctx):
    rng = np.random.default_rng(10)
    k = 10
    keys = np.arange(1 << 20, dtype=np.uint64)
    counts = rng.integers(0, 1 << 32, size=len(keys), dtype=np.uint64).astype(np.uint32)  # sums wrap
    lst = ctx.upload(make_records(keys, counts), k)
    ix = lst.query_index()
    words = rng.integers(0, 1 << 20, size=1_000_037, dtype=np.uint64)
    for n_mm, pm_3 in ((0, 0), (1, 0), (1, 8), (2, 0), (2, 8)):
        _check(ix, keys, counts, words, k, n_mm, pm_3)
    ix.free()
    # a sparse list at the same word length: only canonical words, so both strands of a query meet the same record
    ck = np.unique(M.canonical_np(keys[rng.random(len(keys)) < 0.3], k))
    cc = rng.integers(0, 9, size=len(ck), dtype=np.uint32)
    l2 = ctx.upload(make_records(ck, cc), k)
    ix = l2.query_index()
    for n_mm, pm_3 in ((0, 0), (1, 0), (2, 3), (3, 2)):
        _check(ix, ck, cc, words[:200_001], k, n_mm, pm_3)
    ix.free()


@pytest.fixture(scope="module")
def iid25(ctx):
    rng = np.random.default_rng(25)
    k = 25
    keys = np.unique(M.canonical_np(rng.integers(0, 1 << 50, size=10_300_000, dtype=np.uint64), k))
    assert len(keys) >= 10_000_000
    counts = rng.integers(1, 200, size=len(keys), dtype=np.uint32)
    counts[::1000] = 0
    counts[1::1000] = 0xFFFFFFFF
    lst = ctx.upload(make_records(keys, counts), k)
    n = 1_000_037
    words = rng.integers(0, 1 << 50, size=n, dtype=np.uint64)
    planted = rng.choice(n, size=30_000, replace=False)
    src = keys[rng.integers(0, len(keys), size=len(planted))]
    for j in range(len(planted)):  # one or two substitutions, anywhere; every other one on the other strand
        w = int(src[j])
        for p in rng.choice(k, size=1 + j % 2, replace=False):
            w ^= int(rng.integers(1, 4)) << (2 * int(p))
        words[planted[j]] = M.revcomp(w, k) if j % 4 >= 2 else w
    words[planted[:100]] = src[:100]  # exact
    return k, keys, counts, lst, words, planted


def test_iid_k25(ctx, iid25):
    k, keys, counts, lst, words, planted = iid25
    ix = lst.query_index()
    rng = np.random.default_rng(1)
    _, f0 = _check(ix, keys, counts, words, k, 0, 0)
    assert f0.sum() >= 100
    for pm_3 in (0, 8):
        v1, f1 = _check(ix, keys, counts, words, k, 1, pm_3)
        assert f1.sum() > 1000
    sample = np.unique(np.concatenate([planted, rng.choice(len(words), size=20_000, replace=False), [0, 1, 63, 64, len(words) - 1]]))
    for pm_3 in (0, 8):
        v2, f2 = _check(ix, keys, counts, words, k, 2, pm_3, sample)
        assert f2.sum() > 10_000 or pm_3
    # batches that end inside a wavefront, of size 0 and 1
    for n in (0, 1, 63, 64, 65, 4097):
        w = words[planted[:n]] if n else words[:0]
        for n_mm in (0, 1, 2):
            _check(ix, keys, counts, w, k, n_mm, 0)
    # not canonized: the words as they are
    val, found = ix.lookup(words[:50_000], 0, 0, canonize=False)
    ev, ef = M.lookup_np(keys, counts, words[:50_000], k, 0, 0, canonize=False)
    assert (val == ev).all() and (found == ef).all()
    ix.free()


def test_lookup_all_hits_and_order(ctx, iid25):
    k, keys, counts, lst, words, planted = iid25
    ix = lst.query_index()
    w = words[planted[:3000]]
    for n_mm, pm_3 in ((0, 0), (1, 0), (2, 0), (2, 8)):
        hits = ix.lookup_all(w, n_mm, pm_3, capacity=16)  # too small at first: the call is repeated
        assert (np.diff(hits["query"].astype(np.int64)) >= 0).all()
        q = M.canonical_np(w, k)
        masks = np.array([capi.query_variant_mask(k, n_mm, pm_3, int(r)) for r in np.unique(hits["rank"])], dtype=np.uint64)
        by_rank = dict(zip(np.unique(hits["rank"]).tolist(), masks.tolist()))
        m = np.array([by_rank[int(r)] for r in hits["rank"]], dtype=np.uint64)
        assert (M.canonical_np(q[hits["query"]] ^ m, k) == hits["word"]).all()
        present, cnt = M.find_np(keys, counts, hits["word"])
        assert present.all() and (cnt == hits["count"]).all()
        # the sums of the hits are the lookup's values, and nothing is missing: the hit count per query is the model's
        val, _ = ix.lookup(w, n_mm, pm_3)
        tot = np.zeros(len(w), dtype=np.uint64)
        np.add.at(tot, hits["query"].astype(np.int64), hits["count"].astype(np.uint64))
        assert ((tot & np.uint64(0xFFFFFFFF)).astype(np.uint32) == val).all()
        # the model's print order, query by query: sorting a query's hits by their substitutions (position, value) with
        # a prefix before its extensions must give the model's sequence
        for i in range(0, 3000, 150):
            mine = hits[hits["query"] == i]
            seqs = sorted((tuple((p, (by_rank[int(r)] >> (2 * p)) & 3) for p in range(k) if (by_rank[int(r)] >> (2 * p)) & 3), int(wd), int(c))
                          for r, wd, c in zip(mine["rank"], mine["word"], mine["count"]))
            exp, _ = M.lookup_all(mine["word"], mine["count"], int(w[i]), k, n_mm, pm_3)
            assert [(wd, c) for _, wd, c in seqs] == exp, (i, n_mm, pm_3)
    assert capi.query_variants(k, 2, 8) == M.n_variants(k, 2, 8)
    ix.free()


def test_lookup_all_of_more_tiles_than_two_rounds_of_the_scan(ctx):
    """The scan of the tiles' hit counts (k_tile_scan: one workgroup, rounds of 1024 tiles with the sum so far carried
    from round to round): a batch of 2 x 1024 x 2048 + 3 words is 2049 tiles of 2048 words -- two full rounds and a
    third of one tile.  Exact lookups against a list of a few thousand words; about half of the queries hit."""
    rng = np.random.default_rng(2049)
    k = 16
    keys = np.unique(M.canonical_np(rng.integers(0, 1 << 32, size=5000, dtype=np.uint64), k))
    counts = rng.integers(1, 200, size=len(keys), dtype=np.uint32)
    n = 2 * 1024 * 2048 + 3
    words = rng.integers(0, 1 << 32, size=n, dtype=np.uint64)
    take = rng.random(n) < 0.5
    words[take] = keys[rng.integers(0, len(keys), size=int(take.sum()))]
    words[[0, n - 1]] = keys[[1, 2]]
    lst = ctx.upload(make_records(keys, counts), k)
    ix = lst.query_index()
    try:
        hits = ix.lookup_all(words, 0, 0, capacity=n)
    finally:
        ix.free()
        lst.free()
    val, found = M.lookup_np(keys, counts, words, k, 0, 0)
    at = np.flatnonzero(found)
    assert len(at) > n // 4 and len(hits) == len(at)
    assert (hits["query"] == at.astype(np.uint64)).all()
    assert (hits["rank"] == 0).all()
    assert (hits["word"] == M.canonical_np(words[at], k)).all()
    assert (hits["count"] == val[at]).all()


def test_k32_extreme_keys(ctx):
    rng = np.random.default_rng(32)
    k = 32
    body = rng.integers(0, 1 << 63, size=10_000_000, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=10_000_000, dtype=np.uint64)
    keys = np.unique(np.concatenate([body, np.array([0, 0xFFFFFFFFFFFFFFFF, 1, 0xFFFFFFFFFFFFFFFE], dtype=np.uint64)]))
    counts = rng.integers(1, 9, size=len(keys), dtype=np.uint32)
    lst = ctx.upload(make_records(keys, counts), k)
    ix = lst.query_index()
    words = np.concatenate([np.array([0, 0xFFFFFFFFFFFFFFFF, 3, 1 << 62, 0xFFFFFFFFFFFFFFFC], dtype=np.uint64), keys[::997][:5000], body[:20_000] ^ np.uint64(1 << 40)])
    for n_mm, pm_3 in ((0, 0), (1, 0), (1, 8), (2, 0), (2, 30)):
        val, found = _check(ix, keys, counts, words, k, n_mm, pm_3)
        assert found[0] and found[1]
    with pytest.raises(capi.Gt4HipError):
        ix.lookup(words, 3, 30)  # n_mm + pm_3 > k
    ix.free()


def test_statistics_on_1e8_records(ctx):
    rng = np.random.default_rng(8)
    n, k = 100_000_000, 25
    rec = np.zeros(n, dtype=capi.RECORD_DTYPE)
    rec["key"] = np.arange(n, dtype=np.uint64) * np.uint64(11_000_000) + np.uint64(12345)
    c = rng.integers(1, 300, size=n, dtype=np.uint32)
    big = rng.choice(n, size=1000, replace=False)
    c[big] = rng.integers(1 << 31, 1 << 32, size=1000, dtype=np.uint64).astype(np.uint32)
    c[big[0]] = 0xFFFFFFFF
    c[big[1:50]] = 0
    rec["count"] = c
    lst = ctx.upload(rec, k)
    assert lst.count_stats() == (0, 0xFFFFFFFF)
    for med in (0, 1, 150, 299, 1 << 31, 0xFFFFFFFF):
        assert lst.count_split(med) == (int((c < med).sum()), int((c > med).sum())), med
    for mx in (1, 300, 4096, 5000):
        exp = np.bincount(c[(c >= 1) & (c <= mx)], minlength=mx + 1)[1:mx + 1]
        assert (lst.count_histogram(mx) == exp.astype(np.uint64)).all(), mx
    w = rec["key"]
    x = (w ^ (w >> np.uint64(1))) & np.uint64(0x5555555555555555) & np.uint64((1 << 50) - 1)
    pop = np.zeros(n, dtype=np.uint64)
    for s in range(0, 50, 2):
        pop += (x >> np.uint64(s)) & np.uint64(1)
    assert lst.gc() == int((pop * c.astype(np.uint64)).sum(dtype=np.uint64))
    # a list that does not start on a 16-byte boundary and is no multiple of four records long: the scalar path
    odd = lst.slice(1, 1_000_003)
    co = c[1:1_000_004]
    assert odd.count_stats() == (int(co.min()), int(co.max()))
    assert odd.count_split(150) == (int((co < 150).sum()), int((co > 150).sum()))
    assert odd.gc() == int((pop[1:1_000_004] * co.astype(np.uint64)).sum(dtype=np.uint64))
    empty = ctx.upload(rec[:0], k)
    assert empty.count_stats() == (0xFFFFFFFF, 0) and empty.count_split(3) == (0, 0) and empty.gc() == 0


def test_binary_against_the_reference_binary_live():
    ref = os.path.join(ROOT, "oracle", "_ref", "glistquery")
    if not os.path.exists(ref):
        pytest.skip("oracle/_ref/glistquery is not built")
    rng = np.random.default_rng(99)
    k = 25
    genome = "".join("ACGT"[i] for i in rng.integers(0, 4, size=400_000))
    g = np.frombuffer(genome.encode(), dtype=np.uint8)
    code = np.zeros(256, dtype=np.uint64)
    code[ord("C")], code[ord("G")], code[ord("T")] = 1, 2, 3
    v = code[g]
    w = np.zeros(len(g) - k + 1, dtype=np.uint64)
    for i in range(k):
        w = (w << np.uint64(2)) | v[i:len(g) - k + 1 + i]
    keys = np.unique(M.canonical_np(w[::2], k))
    with tempfile.TemporaryDirectory(prefix="gt4gq_live_") as d:
        write_list(os.path.join(d, "L.list"), make_records(keys, rng.integers(1, 9, size=len(keys), dtype=np.uint32)), k)
        reads = []
        for r in range(1000):
            p = int(rng.integers(0, len(genome) - 125))
            s = list(genome[p:p + 125])
            for q in rng.choice(125, size=3, replace=False):
                s[q] = "ACGTN"[int(rng.integers(0, 5))]
            reads.append(">r%d\n%s\n" % (r, "".join(s)))
        open(os.path.join(d, "reads.fa"), "w").write("".join(reads))
        for extra in (["-mm", "1"], ["-mm", "1", "--all", "-min", "1"]):
            argv = ["L.list", "-s", "reads.fa"] + extra
            a = subprocess.run([ref] + argv, cwd=d, capture_output=True, timeout=600)
            b = subprocess.run([os.path.join(ROOT, "genometester4_amd", "glistquery")] + argv, cwd=d, capture_output=True, timeout=600)
            assert a.returncode == b.returncode == 0, b.stderr
            assert len(a.stdout) > 1_000_000 or "--all" in extra
            assert a.stdout == b.stdout
