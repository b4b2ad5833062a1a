"""tests/hamming_model.py (the reference that sums over keys) held to the two models that enumerate every variant,
tests/query_model.py and tests/mismatch_model.py, at word lengths where enumeration is cheap: k <= 7, up to n_mm == k.
No GPU: what the deep GPU tests (tests/test_mismatch_depth_gpu.py) are checked against is checked here."""
import numpy as np
import pytest

import hamming_model as H
import mismatch_model as MM
import mismatch_util as MU
import query_model as QM


def _list(rng, k, p):
    """a random share p of all 4^k words (so: non-canonical keys and, at even k, palindromes), full-range u32 counts with
    0 and 0xFFFFFFFF among them"""
    space = np.arange(1 << (2 * k), dtype=np.uint64)
    keys = space[rng.random(len(space)) < p]
    counts = rng.integers(0, 1 << 32, size=len(keys), dtype=np.uint64).astype(np.uint32)
    counts[rng.random(len(keys)) < 0.1] = 0
    counts[rng.random(len(keys)) < 0.1] = 0xFFFFFFFF
    return keys, counts


def _words(rng, k, n=300):
    space = 1 << (2 * k)
    return np.arange(space, dtype=np.uint64) if space <= n else rng.integers(0, space, size=n, dtype=np.uint64)


QUERY_SETS = [(1, 1, 0), (2, 2, 0), (3, 3, 0), (4, 2, 1), (5, 3, 2), (5, 5, 0), (6, 2, 0), (6, 6, 0), (7, 3, 4)]


@pytest.mark.parametrize("k,n_mm,pm_3", QUERY_SETS)
def test_lookup_matches_enumeration(k, n_mm, pm_3):
    rng = np.random.default_rng(1000 * k + 10 * n_mm + pm_3)
    words = _words(rng, k)
    for p in (0.5, 1.0, 0.05):
        keys, counts = _list(rng, k, p)
        if k % 2 == 0 and p == 0.5:  # a palindrome, its count neither 0 nor a multiple of 2^31
            half = int(rng.integers(0, 1 << k))  # k / 2 bases, then their reverse complement
            pal = np.uint64((half << k) | QM.revcomp(half, k // 2))
            assert QM.revcomp(int(pal), k) == int(pal)
            keys = np.union1d(keys, [pal])
            counts = np.resize(counts, len(keys))
            counts[np.searchsorted(keys, pal)] = 7
        for canonize in (True, False):
            exp, _ = QM.lookup_np(keys, counts, words, k, n_mm, pm_3, canonize)
            got = H.lookup(keys, counts, words, k, n_mm, pm_3, canonize)
            assert np.array_equal(got, exp), (k, n_mm, pm_3, p, canonize)
    # n_mm == 0 (the exact lookup, pm_3 without effect) and the empty list
    keys, counts = _list(rng, k, 0.5)
    assert np.array_equal(H.lookup(keys, counts, words, k, 0, pm_3), QM.lookup_np(keys, counts, words, k, 0, 0)[0])
    assert not H.lookup(keys[:0], counts[:0], words, k, n_mm, pm_3).any()
    assert len(H.lookup(keys, counts, words[:0], k, n_mm, pm_3)) == 0


def test_the_parameter_sets_reach_the_edges():
    assert any(n_mm == k and pm_3 == 0 for k, n_mm, pm_3 in QUERY_SETS)
    assert any(n_mm + pm_3 == k and pm_3 for k, n_mm, pm_3 in QUERY_SETS)
    assert any(k % 2 == 0 for k, _, _ in QUERY_SETS) and any(k % 2 for k, _, _ in QUERY_SETS)


@pytest.mark.parametrize("k", [1, 2, 5, 6])
def test_closed_form_of_all_variants(k):
    """n_mm == k, pm_3 == 0: every word is a variant of every query, so every query gets the counts of all canonical keys,
    twice (both strands are variants) unless the key is its own reverse complement"""
    rng = np.random.default_rng(k)
    keys, counts = _list(rng, k, 0.6)
    rc = QM.revcomp_np(keys, k)
    total = int((counts[keys < rc].astype(np.uint64) * np.uint64(2)).sum(dtype=np.uint64) + counts[keys == rc].astype(np.uint64).sum(dtype=np.uint64)) & 0xFFFFFFFF
    words = _words(rng, k, 64)
    assert (H.lookup(keys, counts, words, k, k, 0) == total).all()
    assert (QM.lookup_np(keys, counts, words, k, k, 0)[0] == total).all()
    flat = int(counts.astype(np.uint64).sum(dtype=np.uint64)) & 0xFFFFFFFF  # not canonized: every key once
    assert (H.lookup(keys, counts, words, k, k, 0, canonize=False) == flat).all()


@pytest.mark.parametrize("k,c,subtract", [(4, 2, False), (5, 3, True), (6, 4, False), (6, 2, True), (3, 3, True), (5, 5, False)])
def test_level_sums_match_enumeration(k, c, subtract):
    rng = np.random.default_rng(100 * k + 10 * c + subtract)
    words = _words(rng, k, 200)
    empty = np.zeros(0, dtype=np.uint64)
    for p_m, p_q in ((0.3, 0.3), (0.05, 0.6), (0.6, 0.05), (1.0, 0.5)):
        m, _ = _list(rng, k, p_m)
        q, _ = _list(rng, k, p_q)
        q = np.union1d(q, m[::3])  # keys of both lists
        for mk, qk in ((m, q), (m, None), (empty, q), (m, empty), (empty, empty)):
            exp = MM.level_sums(words, k, c, mk, qk, subtract)
            got = H.level_sums(words, k, c, mk, qk, subtract)
            assert got.dtype == exp.dtype and np.array_equal(got, exp), (k, c, subtract, p_m, p_q, len(mk))
    if subtract:  # both rules were seen: a dropped word, and a word with -neg
        s = H.level_sums(words, k, c, m, q, True)
        assert (s == 0xFFFFFFFF).any()
        s = H.level_sums(words, k, c, m[:0], q, True)
        assert ((s > 1 << 31) & (s < 0xFFFFFFFF)).any()
    assert not H.level_sums(words, k, k + 1, m, q, subtract).any()  # above k a level has no variants


@pytest.mark.parametrize("k,n,cutoff,subtract,ddiff", [
    (4, 1, 1, False, True), (4, 2, 2, True, True), (5, 3, 1, False, False), (5, 2, 3, True, False), (6, 1, 0, False, True),
    (4, 6, 1, False, True), (5, 1, 4294967295, True, True), (6, 2, 2, False, True), (5, 5, 40, False, True), (6, 4, 30, True, True),
    (3, 3, 5, True, True)])
def test_compare_mismatch_matches_enumeration(k, n, cutoff, subtract, ddiff):
    a, b = MU.dense_pair(100 + k * 10 + n, k, 0.3, 0.35)
    pairs = [(a, b), (a[:0], b), (a, b[:0]), (a, a)]
    if k == 5:
        pairs.append(MU.planted_pair(5, k, 300))
    for x, y in pairs:
        exp = MM.compare_mismatch(x, y, k, n, cutoff, subtract, ddiff)
        got = H.compare_mismatch(x, y, k, n, cutoff, subtract, ddiff)
        assert exp.keys() == got.keys()
        for bit in exp:
            assert got[bit].tobytes() == exp[bit].tobytes(), (bit, len(got[bit]), len(exp[bit]))
