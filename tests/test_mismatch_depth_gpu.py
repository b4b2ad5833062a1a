"""Mismatch lookups beyond three substitutions: both instantiations of the query kernel and of the level kernel (32-bit
and 64-bit unranking of the variant rank), the level kernel without its early exit, the unranking loop up to eleven and
sixteen substitutions deep, the guards of the entry points and the edges of the bucket index.

Expectations come from tests/hamming_model.py, which sums over the keys of the list instead of enumerating variants
(tests/test_hamming_model.py holds it to the enumeration models), and from those models themselves where they are still
feasible.  Which kernel ran is read from the counters "query_wide", "mm_wide_levels" and "mm_unskipped_levels": the
switch depends on the grid, so on the device, and a test aimed at one side of it must not pass on the other.

The word lengths and mismatch numbers are what puts a case on its side of the switch; the lists, query batches and tables
are as small as they can be (every variant of every query or table word is probed whatever the list holds)."""
import time
from math import comb

import numpy as np
import pytest

import hamming_model as H
import mismatch_model as MM
import query_model as QM
from genometester4_amd import capi
from genometester4_amd.listio import make_records

pytestmark = pytest.mark.gpu
U32 = 0xFFFFFFFF


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _space(k):
    return 1 << (2 * k)


def _random_words(rng, n, k):
    if k == 32:
        return rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=n, dtype=np.uint64)
    return rng.integers(0, _space(k), size=n, dtype=np.uint64)


def _random_canonical(rng, n, k):
    return np.unique(QM.canonical_np(_random_words(rng, n, k), k))


def _counts(rng, n):
    """full-range u32 counts (sums wrap) with 0 and 0xFFFFFFFF among them"""
    c = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    c[::7] = 0
    c[3::11] = U32
    return c


def _mutate(rng, word, positions):
    w = int(word)
    for p in positions:
        w ^= int(rng.integers(1, 4)) << (2 * int(p))
    return w


def _palindrome(rng, k):
    half = int(rng.integers(0, 1 << k))  # k / 2 bases, then their reverse complement
    w = (half << k) | QM.revcomp(half, k // 2)
    assert QM.revcomp(w, k) == w
    return w


def _closed_form(keys, counts, k):
    """n_mm == k, pm_3 == 0: every word is a variant, so every canonical key is found once by each of its strands"""
    rc = QM.revcomp_np(keys, k)
    c = counts.astype(np.uint64)
    return int(c[keys < rc].sum(dtype=np.uint64) * np.uint64(2) + c[keys == rc].sum(dtype=np.uint64)) & U32


def _lookup(ctx, ix, words, n_mm, pm_3=0, canonize=True, wide=None):
    t0 = time.perf_counter()
    val, found = ix.lookup(words, n_mm, pm_3, canonize=canonize)
    print("lookup k=%d n_mm=%d pm_3=%d queries=%d: %.3f s wall, %.1f ms device, query_wide=%d"
          % (ix.list.word_length, n_mm, pm_3, len(words), time.perf_counter() - t0, ix.last_ms, ctx.get_counter("query_wide")))
    if wide is not None:
        assert ctx.get_counter("query_wide") == wide
    assert np.array_equal(found, val != 0) or n_mm == 0
    return val


# ------------------------------------------------------------------ a. the unranking at depth, small k

@pytest.mark.parametrize("k,pm_3", [(6, 0), (8, 0), (6, 3), (8, 3)])
def test_unranking_is_a_bijection_at_depth(ctx, k, pm_3):
    """n_mm == k - pm_3 on a list of every canonical word: every variant of every query is a hit, so the hits are the
    whole (query, rank) space and show what the device made of every rank, up to eight substitutions deep"""
    n_mm, kp = k - pm_3, k - pm_3
    rng = np.random.default_rng(10 * k + pm_3)
    space = np.arange(_space(k), dtype=np.uint64)
    keys = space[space <= QM.revcomp_np(space, k)]
    counts = _counts(rng, len(keys))
    queries = np.concatenate([rng.integers(0, _space(k), size=67, dtype=np.uint64),
                              np.array([0, _space(k) - 1, _palindrome(rng, k)], dtype=np.uint64)])
    nq, V = len(queries), _space(kp)
    assert capi.query_variants(k, n_mm, pm_3) == V == QM.n_variants(k, n_mm, pm_3)
    ix = ctx.upload(make_records(keys, counts), k).query_index()
    t0 = time.perf_counter()
    hits = ix.lookup_all(queries, n_mm, pm_3, capacity=nq * V)
    print("lookup_all k=%d n_mm=%d pm_3=%d: %d hits, %.3f s wall, %.1f ms device" % (k, n_mm, pm_3, len(hits), time.perf_counter() - t0, ix.last_ms))
    assert len(hits) == nq * V
    order = hits["query"].astype(np.int64) * V + hits["rank"].astype(np.int64)
    assert (hits["query"] < nq).all() and (hits["rank"] < V).all() and (np.diff(order) > 0).all()
    masks = np.array([capi.query_variant_mask(k, n_mm, pm_3, r) for r in range(V)], dtype=np.uint64)
    q = QM.canonical_np(queries, k)
    variants = q[:, None] ^ masks[None, :]
    assert np.array_equal(QM.canonical_np(variants.ravel(), k), hits["word"])
    # every word that agrees with the query on its protected bases, each once
    low = np.uint64((1 << (2 * pm_3)) - 1)
    every = (np.arange(V, dtype=np.uint64) << np.uint64(2 * pm_3))[None, :] | (q & low)[:, None]
    assert np.array_equal(np.sort(variants, axis=1), every)
    assert np.array_equal(counts[np.searchsorted(keys, hits["word"])], hits["count"])
    assert not hits["reserved"].any()
    # the sums of the same space
    val = _lookup(ctx, ix, queries, n_mm, pm_3, wide=0)
    assert np.array_equal(val, H.lookup(keys, counts, queries, k, n_mm, pm_3))
    if pm_3 == 0:
        assert (val == _closed_form(keys, counts, k)).all()
    if k == 6:
        assert np.array_equal(val, QM.lookup_np(keys, counts, queries, k, n_mm, pm_3)[0])
    ix.free()


def test_variant_counts_fit_64_bits_or_are_refused():
    refused = []
    for k in (1, 2, 16, 31, 32):
        for n_mm in range(0, 34):
            for pm_3 in range(0, k + 1):
                valid = n_mm <= 32 and not (n_mm and n_mm + pm_3 > k)
                exp = QM.n_variants(k, n_mm, pm_3 if n_mm else 0) if valid else None
                if exp is not None and exp < 1 << 64:
                    assert capi.query_variants(k, n_mm, pm_3) == exp, (k, n_mm, pm_3)
                else:
                    with pytest.raises(capi.Gt4HipError) as e:
                        capi.query_variants(k, n_mm, pm_3)
                    assert e.value.code == capi.EINVAL
                    if valid:
                        refused.append((k, n_mm, pm_3))
    assert refused == [(32, 32, 0)]  # 4^32 variants
    assert capi.query_variants(32, 31, 0) == (1 << 64) - 3 ** 32
    assert capi.query_variants(16, 16, 0) == 1 << 32 and capi.query_variants(16, 15, 0) == 4_251_920_575
    assert capi.query_variants(18, 11, 0) == capi.query_variants(32, 11, 14) == 9_550_961_560


# ------------------------------------------------------------------ b, c. the two query kernels around their switch

@pytest.fixture(scope="module")
def list16(ctx):
    """~20,000 random canonical 16-mers, a palindrome, key 0 and key 4^16 - 1 (all T: not canonical, found only without
    canonisation)"""
    k = 16
    rng = np.random.default_rng(16)
    pal = _palindrome(rng, k)
    keys = np.union1d(_random_canonical(rng, 20_000, k), np.array([0, _space(k) - 1, pal], dtype=np.uint64))
    counts = _counts(rng, len(keys))
    counts[np.searchsorted(keys, np.array([0, _space(k) - 1, pal], dtype=np.uint64))] = (5, 1 << 20, 7)
    assert (counts == 0).any() and (counts == U32).any()
    # a word that is not canonical, the palindrome, and poly-A
    w = int(rng.integers(0, _space(k)))
    queries = np.array([max(w, QM.revcomp(w, k)), pal, 0], dtype=np.uint64)
    ix = ctx.upload(make_records(keys, counts), k).query_index()
    return k, keys, counts, queries, ix


def test_narrow_query_kernel_at_the_top_of_its_range(ctx, list16):
    """k = 16, n_mm = 15: 4^16 - 3^16 = 4,251,920,575 variants per query; ranks pass 2^31 and stay 32-bit"""
    k, keys, counts, queries, ix = list16
    exp = H.lookup(keys, counts, queries, k, 15)
    # the keys sixteen substitutions away are what is NOT found: the values differ from "everything"
    assert (exp != _closed_form(keys, counts, k)).all() and len(set(exp.tolist())) == 3
    val = _lookup(ctx, ix, queries, 15, wide=0)
    assert np.array_equal(val, exp), (val, exp)


def test_wide_query_kernel_just_over_the_switch(ctx, list16):
    """k = 16, n_mm = 16: exactly 2^32 variants per query"""
    k, keys, counts, queries, ix = list16
    exp = H.lookup(keys, counts, queries, k, 16)
    assert (exp == _closed_form(keys, counts, k)).all()
    val = _lookup(ctx, ix, queries, 16, wide=1)
    assert np.array_equal(val, exp), (val, exp)


def test_wide_query_kernel_without_canonisation(ctx, list16):
    """canonize = 0: every key is found once, by itself -- the non-canonical key too"""
    k, keys, counts, queries, ix = list16
    exp = H.lookup(keys, counts, queries[:2], k, 16, canonize=False)
    assert (exp == (int(counts.astype(np.uint64).sum(dtype=np.uint64)) & U32)).all()
    assert (exp != _closed_form(keys, counts, k)).all()
    val = _lookup(ctx, ix, queries[:2], 16, canonize=False, wide=1)
    assert np.array_equal(val, exp), (val, exp)


def _planted_list(rng, k, queries, n_random, n_mm, pm_3):
    """random canonical keys, and around every query (canonical form) words 0 .. n_mm + 2 substitutions away at the
    positions that may change, and words within n_mm with one protected base changed as well"""
    plant = []
    for q in QM.canonical_np(queries, k).tolist():
        for d in range(0, n_mm + 3):
            for _ in range(40 if d == n_mm else 2):  # the deepest level holds the highest ranks: sample it well
                plant.append(_mutate(rng, q, pm_3 + rng.choice(k - pm_3, size=d, replace=False)))
        for d in range(0, min(n_mm, 3) if pm_3 else 0):
            plant.append(_mutate(rng, q, np.append(pm_3 + rng.choice(k - pm_3, size=d, replace=False), rng.integers(0, pm_3))))
    keys = np.union1d(_random_canonical(rng, n_random, k), QM.canonical_np(np.array(plant, dtype=np.uint64), k))
    return keys, _counts(rng, len(keys))


def test_wide_query_kernel_k32_with_protected_bases(ctx):
    """k = 32, n_mm = 11, pm_3 = 14: 9,550,961,560 variants over the 18 high bases, masks shifted by 28 bits, keys with
    bit 63 set; the second query is not canonical and is looked up by its reverse complement"""
    k, n_mm, pm_3 = 32, 11, 14
    rng = np.random.default_rng(32)
    c = _random_canonical(rng, 64, k)
    high = c[(c >> np.uint64(63)) == 1]
    queries = np.array([high[0], QM.revcomp(int(c[1]), k)], dtype=np.uint64)
    assert QM.canonical(int(queries[1]), k) != int(queries[1])
    keys, counts = _planted_list(rng, k, queries, 20_000, n_mm, pm_3)
    assert ((keys >> np.uint64(63)) == 1).sum() > 1000
    exp = H.lookup(keys, counts, queries, k, n_mm, pm_3)
    near = H.lookup(keys, np.ones(len(keys), dtype=np.uint32), queries, k, n_mm, pm_3)
    loose = H.lookup(keys, np.ones(len(keys), dtype=np.uint32), queries, k, n_mm + 2, 0)
    assert (near >= 2 * n_mm + 38).all() and (loose > near + 4).all()  # planted words are found, and planted words are not
    ix = ctx.upload(make_records(keys, counts), k).query_index()
    val = _lookup(ctx, ix, queries, n_mm, pm_3, wide=1)
    assert np.array_equal(val, exp), (val, exp)
    ix.free()


def test_wide_query_kernel_k18_batch_crosses_queries(ctx):
    """k = 18, n_mm = 11: the same 9,550,961,560 variants without a shift; three queries, so the grid's stride carries
    from one query into the next twice"""
    k, n_mm = 18, 11
    rng = np.random.default_rng(18)
    queries = _random_words(rng, 3, k)
    keys, counts = _planted_list(rng, k, queries, 20_000, n_mm, 0)
    exp = H.lookup(keys, counts, queries, k, n_mm)
    near = H.lookup(keys, np.ones(len(keys), dtype=np.uint32), queries, k, n_mm)
    assert (near > 1000).all() and (near < len(keys)).all()  # random 18-mers lie 13.5 bases apart: a share is in reach
    ix = ctx.upload(make_records(keys, counts), k).query_index()
    val = _lookup(ctx, ix, queries, n_mm, wide=1)
    assert np.array_equal(val, exp), (val, exp)
    ix.free()


# ------------------------------------------------------------------ d. gt4hip_compare_mismatch through a 64-bit level

BIG = 1_000_000  # the count of a word that is to enter a table (>= every cutoff here)


def _plain_case(seed, k, n_b, n_table, n_dd=0):
    """B: n_b random canonical keys with small counts.  A: B's keys with count 1 (below the cutoff: none of them enters
    the diff1 table) and n_table other words with count BIG, which are the diff1 table.  n_dd keys of B have count BIG
    there: they are the diff2 table (-dd).  Returns (a, b, the diff1 table's keys)."""
    rng = np.random.default_rng(seed)
    kb = _random_canonical(rng, n_b, k)
    extra = np.setdiff1d(_random_words(rng, n_table, k), kb)
    assert len(extra) == n_table
    ka = np.union1d(kb, extra)
    ca = np.where(np.isin(ka, extra), BIG, 1).astype(np.uint32)
    cb = rng.integers(1, 5, size=len(kb), dtype=np.uint32)
    cb[rng.choice(len(kb), size=n_dd, replace=False)] = BIG
    return make_records(ka, ca), make_records(kb, cb), extra


def _levels(table_keys, k, n, cutoff, m_keys, q_keys, subtract):
    """[(words alive at level c, their s)] for c = 1..n by the Hamming reference"""
    out, t = [], np.asarray(table_keys, dtype=np.uint64)
    for c in range(1, n + 1):
        s = H.level_sums(t, k, c, m_keys, q_keys, subtract)
        out.append((t, s))
        t = t[s < cutoff]
    return out


def _run_mm(ctx, a, b, k, n, cutoff, subtract=False, ddiff=False, count_only_too=False):
    ops = capi.OP_DIFF1 | (capi.OP_DIFF2 if ddiff else 0)
    exp = H.compare_mismatch(a, b, k, n, cutoff, subtract, ddiff)
    da, db = ctx.upload(a, k), ctx.upload(b, k)
    t0 = time.perf_counter()
    st, out, timing = ctx.compare_mismatch(da, db, ops, n, cutoff=cutoff, subtract=subtract)
    wall = time.perf_counter() - t0
    counters = ctx.get_counter("mm_wide_levels"), ctx.get_counter("mm_unskipped_levels")
    print("compare_mismatch k=%d -mm %d cutoff=%d subtract=%d dd=%d: %.3f s wall, level words %s, wide/unskipped levels %s"
          % (k, n, cutoff, subtract, ddiff, wall, timing["level_words"], counters))
    for bit, rec in exp.items():
        got = out[bit].download()
        assert got.tobytes() == rec.tobytes(), (bit, got, rec)
        assert st[bit] == MM.totals(rec)
    if count_only_too:
        cst, _, _ = ctx.compare_mismatch(da, db, ops, n, cutoff=cutoff, subtract=subtract, count_only=True)
        assert cst == st
    return exp, timing, counters


K18_SEED, K18_CUTOFF = 1800, 640
K17_SEED, K17_CUTOFF = 1701, 1761
DU_SEED = 17


@pytest.mark.parametrize("ddiff", [False, True], ids=["diff", "dd"])
def test_mismatch_level_with_64_bit_ranks_and_no_early_exit(ctx, ddiff):
    """k = 18, -mm 11: level 10 has 2,583,866,142 variants per word (32-bit kernel), level 11 5,637,526,128 (64-bit
    kernel, and no early exit: a u32 count could wrap).  Four words reach level 11 and two of them fall there."""
    k, n, cutoff = 18, 11, K18_CUTOFF
    a, b, table = _plain_case(K18_SEED, k, 4000, 4, n_dd=2 if ddiff else 0)
    lv = _levels(table, k, n, cutoff, b["key"], None, False)
    assert all(len(t) == 4 for t, _ in lv) and (lv[-1][1] >= cutoff).sum() == 2
    assert max(int(s.max()) for _, s in lv[:-1]) < cutoff and 4 < cutoff <= BIG
    alive = [len(t) for t, _ in lv]
    if ddiff:
        d2 = MM.prepass(a, b, cutoff, False, True)[1]
        assert len(d2) == 2
        alive = [x + len(t) for x, (t, _) in zip(alive, _levels(d2["key"], k, n, cutoff, a["key"], None, False))]
    exp, timing, (wide, unskipped) = _run_mm(ctx, a, b, k, n, cutoff, ddiff=ddiff, count_only_too=not ddiff)
    assert len(exp[4]) == 2
    assert timing["level_words"] == alive
    per_word = comb(18, 11) * 3 ** 11
    assert per_word == 5_637_526_128 and comb(18, 10) * 3 ** 10 == 2_583_866_142
    sides = 1 + (ddiff and alive[-1] > 4)
    assert wide == sides and unskipped == sides
    assert timing["level_probes"][10] == alive[-1] * per_word  # nothing may be skipped


def _subtract_case(seed):
    """-du at k = 18, -mm 11.  B is inside A but for one key.  The table is the four common keys with f1 >= cutoff > f2;
    an A-only key 11 substitutions from table word 0 counts -1 and drops it; an A-only key 12 away from word 1 is out
    of reach; the B-only key 11 away from word 2 kills it; word 3 has nothing near."""
    k, cutoff = 18, 5
    rng = np.random.default_rng(seed)
    common = _random_canonical(rng, 4000, k)
    table = np.sort(rng.choice(common, size=4, replace=False))
    plant = [QM.canonical(_mutate(rng, table[i], rng.choice(k, size=d, replace=False)), k) for i, d in ((0, 11), (1, 12), (2, 11))]
    assert not np.isin(plant, common).any() and len(set(plant)) == 3
    ka = np.union1d(common, np.array(plant[:2], dtype=np.uint64))
    kb = np.union1d(common, np.array(plant[2:], dtype=np.uint64))
    a = make_records(ka, np.where(np.isin(ka, table), 9, 1).astype(np.uint32))
    b = make_records(kb, np.where(np.isin(kb, table), 2, 1).astype(np.uint32))
    return a, b, table, k, cutoff


def test_mismatch_subtract_through_a_64_bit_level(ctx):
    a, b, table, k, cutoff = _subtract_case(DU_SEED)
    n = 11
    d1 = MM.prepass(a, b, cutoff, True, False)[0]
    assert np.array_equal(d1["key"], table) and (d1["count"] == 7).all()
    lv = _levels(table, k, n + 1, 1 << 33, b["key"], a["key"], True)  # (a cutoff nothing reaches: every level on all four)
    assert all(not s.any() for _, s in lv[:10])  # no accidental neighbour within ten
    only_a, only_b = np.setdiff1d(a["key"], b["key"]), np.setdiff1d(b["key"], a["key"])
    assert H.level_sums(table, k, 11, only_b, None, False).tolist() == [0, 0, 1, 0]  # the kill
    assert H.level_sums(table, k, 11, only_a, None, False).tolist() == [1, 0, 0, 0]  # the -1
    assert H.level_sums(table, k, 12, only_a, None, False)[1] >= 1                    # one further: not seen
    assert lv[10][1].tolist() == [U32, 0, U32, 0]
    exp, timing, (wide, unskipped) = _run_mm(ctx, a, b, k, n, cutoff, subtract=True)
    assert np.array_equal(exp[4]["key"], table[[1, 3]])
    assert timing["level_words"] == [4] * 11
    assert wide == 1 and unskipped == 0  # -du keeps the early exit


def test_mismatch_narrow_level_kernel_at_the_top_of_its_range(ctx):
    """k = 17, -mm 13: the largest level has C(17, 13) * 3^13 = 3,794,488,740 variants per word, still 32-bit"""
    k, n, cutoff = 17, 13, K17_CUTOFF
    assert max(comb(k, c) * 3 ** c for c in range(1, n + 1)) == comb(17, 13) * 3 ** 13 == 3_794_488_740
    a, b, table = _plain_case(K17_SEED, k, 4000, 2)
    lv = _levels(table, k, n, cutoff, b["key"], None, False)
    assert all(len(t) == 2 for t, _ in lv) and (lv[-1][1] >= cutoff).sum() == 1  # both reach level 13, one falls there
    exp, timing, (wide, unskipped) = _run_mm(ctx, a, b, k, n, cutoff)
    assert len(exp[4]) == 1
    assert timing["level_words"] == [2] * 13
    assert wide == 0 and unskipped == 0


# ------------------------------------------------------------------ e. the guards

def test_guards_refuse_and_leave_the_context_usable(ctx):
    k = 32
    rng = np.random.default_rng(5)
    keys = _random_canonical(rng, 1000, k)
    counts = rng.integers(1, 9, size=len(keys), dtype=np.uint32)
    ix = ctx.upload(make_records(keys, counts), k).query_index()
    words = np.concatenate([keys[:50], keys[50:100] ^ np.uint64(1 << 40), _random_words(rng, 20, k)])

    def still_answers():
        for n_mm in (0, 1):
            val, found = ix.lookup(words, n_mm)
            ev, ef = QM.lookup_np(keys, counts, words, k, n_mm)
            assert np.array_equal(val, ev) and np.array_equal(found, ef) and found.sum() >= 50

    def refused(text, call):
        with pytest.raises(capi.Gt4HipError) as e:
            call()
        assert e.value.code == capi.EINVAL and text in str(e.value), str(e.value)
        still_answers()

    still_answers()
    refused("more than 2^64 variants", lambda: ix.lookup(words[:3], 32))
    refused("more than 2^64 variants", lambda: ix.lookup_all(words[:1], 32))
    refused("split the batch", lambda: ix.lookup(np.zeros(1_000_000, dtype=np.uint64), 25))
    refused("too many for one call", lambda: ix.lookup_all(words[:1], 16))
    refused("do not fit a word", lambda: ix.lookup(words[:3], 20, 13))
    ix.free()
    # glistcompare -mm 32 at k = 32.  A level is refused ("more than 2^64 variants") when words x variants does not fit
    # 64 bits -- ten words at level 20 and beyond -- but only a level that is RUN is sized, and a table runs level c + 1
    # only with the words that survived level c.  Ten words that each have a key of B one substitution away all fall at
    # level 1: the call succeeds with nothing left, and no later level does any work.
    kb = _random_canonical(rng, 500, k)
    table = np.setdiff1d(np.array([_mutate(rng, w, [rng.integers(0, k)]) for w in kb[:10]], dtype=np.uint64), kb)
    assert len(table) == 10
    ka = np.union1d(kb, table)
    a = make_records(ka, np.where(np.isin(ka, table), BIG, 1).astype(np.uint32))
    b = make_records(kb, np.ones(len(kb), dtype=np.uint32))
    assert np.array_equal(MM.prepass(a, b, 1, False, False)[0]["key"], np.sort(table))
    assert (H.level_sums(np.sort(table), k, 1, kb, None, False) >= 1).all()
    exp, timing, _ = _run_mm(ctx, a, b, k, 32, 1, count_only_too=True)
    assert len(exp[4]) == 0
    assert timing["level_words"] == [10] + [0] * 31 and timing["level_probes"][0] <= 10 * 96 and not any(timing["level_probes"][1:])
    ix = ctx.upload(make_records(keys, counts), k).query_index()
    still_answers()
    ix.free()


# ------------------------------------------------------------------ f. the edges of the bucket index

def _check_enumerated(ix, keys, counts, words, k, hamming=True):
    """n_mm 0 and 1 against the enumeration model (and the Hamming reference, O(words x keys), where that is cheap);
    {n_mm: found}"""
    out = {}
    for n_mm in (0, 1):
        val, found = ix.lookup(words, n_mm)
        ev, ef = QM.lookup_np(keys, counts, words, k, n_mm)
        assert np.array_equal(val, ev) and np.array_equal(found, ef), (k, n_mm, len(keys))
        assert not hamming or np.array_equal(val, H.lookup(keys, counts, words, k, n_mm))
        out[n_mm] = found
    return out


def test_index_of_one_and_two_records(ctx):
    k = 25
    rng = np.random.default_rng(1)
    for n in (1, 2):
        keys = _random_canonical(rng, n, k)
        counts = np.arange(3, 3 + n, dtype=np.uint32)
        near = np.array([_mutate(rng, w, [p]) for w in keys for p in (0, 12, 24)], dtype=np.uint64)
        words = np.concatenate([keys, QM.revcomp_np(keys, k), near, np.array([0, _space(k) - 1], dtype=np.uint64), _random_words(rng, 50, k)])
        ix = ctx.upload(make_records(keys, counts), k).query_index()
        found = _check_enumerated(ix, keys, counts, words, k)
        assert found[0].sum() >= 2 * n and found[1].sum() >= 5 * n
        ix.free()


def test_index_with_every_key_in_one_bucket(ctx):
    """~10^5 keys at k = 25 that share their top 30 bits: the index has 2^13 buckets, all keys but three lie in one of
    them, and the binary search runs over the whole list"""
    k = 25
    rng = np.random.default_rng(2)
    base = np.uint64(0x0123_4567 << 20)
    keys = np.union1d(base | rng.choice(1 << 20, size=100_000, replace=False).astype(np.uint64),
                      np.array([5, (1 << 49) + 12345, (1 << 50) - (1 << 30)], dtype=np.uint64))
    keys = keys[keys <= QM.revcomp_np(keys, k)]  # (a key ending in TT.. here is the larger strand: never looked up)
    assert 90_000 < len(keys) and len(np.unique(keys[1:-2] >> np.uint64(20))) == 1 and len(np.unique(keys >> np.uint64(20))) == 4
    counts = _counts(rng, len(keys))
    pick = keys[rng.choice(len(keys), size=2000, replace=False)]
    near = pick ^ (rng.integers(1, 4, size=len(pick)).astype(np.uint64) << (np.uint64(2) * rng.integers(0, k, size=len(pick)).astype(np.uint64)))
    words = np.concatenate([pick, near, QM.revcomp_np(pick[:100], k), keys[:1], keys[-2:], base | np.arange(64, dtype=np.uint64), _random_words(rng, 200, k)])
    ix = ctx.upload(make_records(keys, counts), k).query_index()
    found = _check_enumerated(ix, keys, counts, words, k, hamming=False)[0]
    assert found[:2000].all() and not found.all()
    ix.free()


def test_index_at_word_length_two(ctx):
    """k = 2 (and 1): the index bits are bounded by 2k; all 16 words, and a list with gaps"""
    rng = np.random.default_rng(3)
    for k in (2, 1):
        words = np.arange(_space(k), dtype=np.uint64)
        for keys in (words, words[[1, 2]] if k == 1 else words[[0, 3, 4, 9, 14]]):
            counts = rng.integers(1, 1 << 32, size=len(keys), dtype=np.uint64).astype(np.uint32)
            ix = ctx.upload(make_records(keys, counts), k).query_index()
            _check_enumerated(ix, keys, counts, words, k)
            val = _lookup(ctx, ix, words, k, wide=0)
            assert np.array_equal(val, H.lookup(keys, counts, words, k, k))
            ix.free()


def test_index_on_a_slice_that_is_not_16_byte_aligned(ctx):
    k = 25
    rng = np.random.default_rng(4)
    keys = _random_canonical(rng, 5003, k)
    counts = _counts(rng, len(keys))
    lst = ctx.upload(make_records(keys, counts), k)
    view = lst.slice(1, len(keys) - 2)
    assert view.device_ptr % 16 == 12
    ix = view.query_index()
    near = keys[:400] ^ np.uint64(2 << 20)
    words = np.concatenate([keys, near, _random_words(rng, 100, k)])
    found = _check_enumerated(ix, keys[1:-1], counts[1:-1], words, k)[0]
    assert not found[0] and not found[len(keys) - 1] and found[1:len(keys) - 1].all()
    ix.free()
