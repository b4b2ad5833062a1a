"""glistquery --per_sequence restated on the CPU: the reader of tests/index_model.py (words and the ordinal of each one's
sequence) and the lookup rule of tests/query_model.py, added up per sequence.  tests/test_gqseq_model.py holds it to
what the reference's own `glistquery -s` prints sequence by sequence, which licenses it as the expectation of the GPU tests."""
import numpy as np

import index_model
import query_model


def hits_np(keys, counts, words, k, n_mm=0, pm_3=0, lo=1, hi=0xFFFFFFFF):
    """(hit, value) per word: a word is a hit when gt4hip_query_lookup finds it and lo <= value <= hi.  Without mismatches
    the word is looked up as it stands (the reader's words are canonical); its variants are canonicalised as ever"""
    words = np.asarray(words, dtype=np.uint64)
    val, found = query_model.lookup_np(np.asarray(keys, dtype=np.uint64), np.asarray(counts, dtype=np.uint32), words, k, n_mm, pm_3, canonize=n_mm > 0)
    val = val.astype(np.uint64)
    return found & (val >= np.uint64(lo)) & (val <= np.uint64(hi)), val


def profile_words(keys, counts, words, ordinals, n_seqs, k, n_mm=0, pm_3=0, lo=1, hi=0xFFFFFFFF, first_ordinal=0):
    """rows of (n_words, n_hits, sum), entry s for the words of ordinal first_ordinal + s (gt4hip_query_profile_words);
    the words are looked up as they stand (the reader's are canonical)"""
    out = np.zeros((n_seqs, 3), dtype=np.uint64)
    if len(words) == 0:
        return out
    hit, val = hits_np(keys, counts, words, k, n_mm, pm_3, lo, hi)
    s = np.asarray(ordinals, dtype=np.int64) - first_ordinal
    out[:, 0] = np.bincount(s, minlength=n_seqs).astype(np.uint64)
    out[:, 1] = np.bincount(s[hit], minlength=n_seqs).astype(np.uint64)
    sums = [0] * n_seqs  # exact: a float bincount would round sums above 2^53
    for i in np.flatnonzero(hit).tolist():
        sums[s[i]] += int(val[i])
    out[:, 2] = np.array([v & 0xFFFFFFFFFFFFFFFF for v in sums], dtype=np.uint64)
    return out


def name_of(text: bytes, name_pos: int) -> bytes:
    """the bytes of a name up to the first one <= ' ' (or the end of the file)"""
    e = name_pos
    while e < len(text) and text[e] > 32:
        e += 1
    return text[name_pos:e]


def profile_text(keys, counts, text: bytes, k, n_mm=0, pm_3=0, lo=1, hi=0xFFFFFFFF):
    """(names, rows of (n_words, n_hits, sum)) of the sequences of one file, in file order"""
    words, ords, _, _, subs = index_model.read_locations(text, k)
    rows = profile_words(keys, counts, np.array(words, dtype=np.uint64), ords, len(subs), k, n_mm, pm_3, lo, hi)
    return [name_of(text, s[0]) for s in subs], rows


def stdout_of(keys, counts, text: bytes, k, n_mm=0, pm_3=0, min_freq=0, max_freq=0xFFFFFFFF, min_hits=0) -> bytes:
    """what `glistquery LIST -s FILE --per_sequence` prints: NAME, WORDS, HITS, SUM per sequence with HITS >= min_hits;
    a hit has max (min_freq, 1) <= value <= max_freq"""
    names, rows = profile_text(keys, counts, text, k, n_mm, pm_3, max(min_freq, 1), max_freq)
    return b"".join(b"%s\t%d\t%d\t%d\n" % (n, int(r[0]), int(r[1]), int(r[2])) for n, r in zip(names, rows) if int(r[1]) >= min_hits)
