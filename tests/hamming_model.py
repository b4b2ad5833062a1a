"""A reference of the mismatch lookups that never enumerates a variant: the sum over the variants of a word is a sum
over the KEYS of the list, so its cost is O(|list|) per word whatever the number of mismatches is.  It is the yardstick
where tests/query_model.py and tests/mismatch_model.py (which enumerate, and which tests/test_hamming_model.py holds
this file to) cannot go: more than three substitutions at k >= 16, variant spaces beyond 2^32.

A variant v of a word q is looked up as canonical (v) = min (v, revcomp (v)), and distinct variants are distinct
words.  So a key x of the list is found exactly by the words v in {x, revcomp (x)} -- and only when x <= revcomp (x): a
non-canonical key is never looked up.  The words that find some key, each with the count it finds, are the list's
EXPANSION; a lookup "up to n_mm mismatches" of q adds the counts of the expansion's words within Hamming distance n_mm
(in bases) of q that agree with q on the pm_3 protected low bases, and level c of glistcompare -mm counts the
expansion's words at distance exactly c.  Without canonisation every key is found by itself alone."""
import numpy as np

import mismatch_model as MM
from query_model import canonical_np, revcomp_np

U32 = 0xFFFFFFFF
_ODD = np.uint64(0x5555555555555555)


def expansion(keys, counts, k, canonize=True):
    """(words, counts): every word whose lookup finds a key of the list, and the count it finds (counts None: ones)"""
    keys = np.asarray(keys, dtype=np.uint64)
    counts = np.ones(len(keys), dtype=np.uint64) if counts is None else np.asarray(counts).astype(np.uint64)
    if not canonize or len(keys) == 0:
        return keys, counts
    rc = revcomp_np(keys, k)
    can, other = keys <= rc, keys < rc  # other: the second strand of a key that is no palindrome
    return np.concatenate([keys[can], rc[other]]), np.concatenate([counts[can], counts[other]])


def distance(a, b):
    """Hamming distance in bases of 2-bit packed words (broadcasts)"""
    t = np.bitwise_xor(a, b)
    return np.bitwise_count((t | (t >> np.uint64(1))) & _ODD)


def _chunks(n_words, n_cols, cells=1 << 22):
    step = max(1, cells // max(1, n_cols))
    return [(i, min(n_words, i + step)) for i in range(0, n_words, step)]


def lookup(keys, counts, words, k, n_mm=0, pm_3=0, canonize=True):
    """the u32 values of gt4hip_query_lookup for an array of query words"""
    words = np.asarray(words, dtype=np.uint64)
    q = canonical_np(words, k) if canonize else words
    ew, ec = expansion(keys, counts, k, canonize)
    out = np.zeros(len(q), dtype=np.uint32)
    if len(ew) == 0:
        return out
    low = np.uint64((1 << (2 * pm_3)) - 1 if n_mm else 0)  # n_mm == 0 is the exact lookup: nothing to protect
    for i, j in _chunks(len(q), len(ew)):
        qq = q[i:j, None]
        near = (distance(ew[None, :], qq) <= n_mm) & (((ew[None, :] ^ qq) & low) == 0)
        out[i:j] = (np.where(near, ec[None, :], np.uint64(0)).sum(axis=1, dtype=np.uint64) & np.uint64(U32)).astype(np.uint32)
    return out


def _at_distance(words, ew, c):
    """per word: how many words of ew lie at distance exactly c"""
    n = np.zeros(len(words), dtype=np.uint64)
    if len(ew):
        for i, j in _chunks(len(words), len(ew)):
            n[i:j] = (distance(ew[None, :], words[i:j, None]) == c).sum(axis=1)
    return n


def level_sums(words, k, c, m_keys, q_keys, subtract):
    """s of every word at level c, as mismatch_model.level_sums gives it: the variants present in m; with subtract
    0xFFFFFFFF for a word with a variant in m and not in q (dropped), else minus the variants in q and not in m."""
    words = np.asarray(words, dtype=np.uint64)
    em, _ = expansion(m_keys, None, k)
    if not subtract:
        return _at_distance(words, em, c) & np.uint64(U32)
    eq, _ = expansion(q_keys if q_keys is not None else np.zeros(0, dtype=np.uint64), None, k)
    drop = _at_distance(words, np.setdiff1d(em, eq), c) != 0
    neg = _at_distance(words, np.setdiff1d(eq, em), c)
    return np.where(drop, np.uint64(U32), (np.uint64(1 << 32) - neg) & np.uint64(U32))


def fetch(table, k, n_mismatch, cutoff, m_keys, q_keys, subtract):
    """survivors of levels 1..N, in table order (above k a level has no variants: one stands for them all)"""
    t = table
    for c in range(1, min(n_mismatch, k + 1) + 1):
        if len(t) == 0:
            break
        t = t[level_sums(t["key"], k, c, m_keys, q_keys, subtract) < cutoff]
    return t


def compare_mismatch(a, b, k, n_mismatch, cutoff=1, subtract=False, ddiff=False):
    """{4: D1 output records, 8: D2 output records (with ddiff)}: mismatch_model's pre-pass, the levels from here"""
    d1, d2 = MM.prepass(a, b, cutoff, subtract, ddiff)
    out = {4: fetch(d1, k, n_mismatch, cutoff, b["key"], a["key"] if subtract else None, subtract)}
    if ddiff:
        out[8] = fetch(d2, k, n_mismatch, cutoff, a["key"], None, subtract)
    return out
