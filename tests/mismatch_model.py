"""A vectorised numpy restatement of glistcompare -mm N (compare_wordmaps_mm, fetch_relevant_words and
search_query of the reference, src/glistcompare.c:958-1168): the model the GPU results are checked against.

Pre-pass: one merge of A (list 1) and B (list 2) gives table D1 (diff) and D2 (-dd); g1 = f1 >= cutoff and
g2 = f2 >= cutoff are taken before -du subtracts f1 from f2.  Levels c = 1..N: every word of a table enumerates
its variants with exactly c substitutions, canonicalises them and counts the ones PRESENT in the other list
(B for D1, A for D2); with subtract a variant present in B and not in A drops the word and one present in A and
not in B counts -1 (mod 2^32); D2 has no second list (its lookups give 0).  A word survives while s < cutoff."""
import itertools

import numpy as np

from genometester4_amd.listio import make_records
from mismatch_util import canonical

U32 = 0xFFFFFFFF


def variant_masks(k, c):
    """XOR masks of every variant with exactly c substituted bases (C(k, c) * 3^c of them)"""
    if c > k:
        return np.zeros(0, dtype=np.uint64)
    out = []
    for pos in itertools.combinations(range(k), c):
        for subs in itertools.product((1, 2, 3), repeat=c):
            m = 0
            for p, s in zip(pos, subs):
                m |= s << (2 * p)
            out.append(m)
    return np.array(out, dtype=np.uint64)


def present(sorted_keys, q):
    """1 where q is a key of the list (an empty list holds nothing)"""
    if len(sorted_keys) == 0:
        return np.zeros(q.shape, dtype=bool)
    idx = np.searchsorted(sorted_keys, q)
    return sorted_keys[np.minimum(idx, len(sorted_keys) - 1)] == q


def prepass(a, b, cutoff, subtract, ddiff):
    """(D1 records, D2 records or None)"""
    ka, fa = a["key"], a["count"].astype(np.uint32)
    kb, fb = b["key"], b["count"].astype(np.uint32)
    common, ia, ib = np.intersect1d(ka, kb, assume_unique=True, return_indices=True)
    f1, f2 = fa[ia], fb[ib].copy()
    g1, g2 = f1 >= np.uint32(cutoff), f2 >= np.uint32(cutoff)
    if subtract:
        f2 = np.where(f1 <= f2, f2 - f1, f2)
    only_a = np.ones(len(ka), dtype=bool)
    only_a[ia] = False
    only_b = np.ones(len(kb), dtype=bool)
    only_b[ib] = False
    keep_c = g1 & ~g2
    keep_a = only_a & (fa >= np.uint32(cutoff)) & (not subtract)
    d1k = np.concatenate([common[keep_c], ka[keep_a]])
    d1f = np.concatenate([(f1 - f2)[keep_c], fa[keep_a]])
    o = np.argsort(d1k, kind="stable")
    d1 = make_records(d1k[o], d1f[o])
    d2 = None
    if ddiff:
        keep_c2 = g2 & ~g1
        keep_b = only_b & (fb >= np.uint32(cutoff))
        d2k = np.concatenate([common[keep_c2], kb[keep_b]])
        d2f = np.concatenate([(f2 - f1)[keep_c2], fb[keep_b]])
        o = np.argsort(d2k, kind="stable")
        d2 = make_records(d2k[o], d2f[o])
    return d1, d2


def level_sums(words, k, c, m_keys, q_keys, subtract, chunk=1 << 22):
    """s of every word at level c (uint64 array holding u32 values)"""
    masks = variant_masks(k, c)
    s = np.zeros(len(words), dtype=np.uint64)
    if len(masks) == 0 or len(words) == 0:
        return s
    step = max(1, chunk // len(masks))
    for i in range(0, len(words), step):
        w = words[i:i + step]
        cv = canonical(w[:, None] ^ masks[None, :], k)
        pm = present(m_keys, cv)
        if subtract:
            pq = present(q_keys, cv) if q_keys is not None else np.zeros_like(pm)
            drop = (pm & ~pq).any(axis=1)
            neg = (pq & ~pm).sum(axis=1).astype(np.uint64)
            s[i:i + step] = np.where(drop, U32, (np.uint64(1 << 32) - neg) & np.uint64(U32))
        else:
            s[i:i + step] = pm.sum(axis=1).astype(np.uint64) & np.uint64(U32)
    return s


def fetch(table, k, n_mismatch, cutoff, m_keys, q_keys, subtract):
    """survivors of levels 1..N, in table order"""
    t = table
    for c in range(1, min(n_mismatch, k + 1) + 1):
        if len(t) == 0:
            break
        s = level_sums(t["key"], k, c, m_keys, q_keys, subtract)
        t = t[s < cutoff]
    return t


def compare_mismatch(a, b, k, n_mismatch, cutoff=1, subtract=False, ddiff=False):
    """{4: D1 output records, 8: D2 output records (with ddiff)}"""
    d1, d2 = prepass(a, b, cutoff, subtract, ddiff)
    out = {4: fetch(d1, k, n_mismatch, cutoff, b["key"], a["key"] if subtract else None, subtract)}
    if ddiff:
        out[8] = fetch(d2, k, n_mismatch, cutoff, a["key"], None, subtract)
    return out


def totals(rec):
    return len(rec), int(rec["count"].astype(np.uint64).sum())
