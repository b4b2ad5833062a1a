"""numpy / Python restatement of glistquery's lookup rule (gt4_word_dict_lookup_mm as search_one_word calls it,
reference src/word-dict.c:74-106, src/glistquery.c:543-568), of the order --all prints variants in (the pre-order of
gt4_word_table_generate_mismatches, src/word-table.c:360-382), of its word parsers and of its statistics: the
independent yardstick of the device code (tests/test_gquery_model.py holds it to the reference's own transcripts)."""
from __future__ import annotations

import itertools

import numpy as np

M64 = (1 << 64) - 1


# ------------------------------------------------------------------ words

def nucl_value(ch: str) -> int:
    """get_nucl_value, src/sequence.c:43-52, on a signed char"""
    c = ord(ch)
    if c >= 128:
        c -= 256
    if c & 4:
        return ((c >> 4) | 2) & 3
    return (c & 6) >> 1


def string_to_word(s: str, k: int) -> int:
    w = 0
    for ch in s[:min(k, 32)]:
        w = ((w << 2) | nucl_value(ch)) & M64
    return w


def word_to_string(w: int, k: int) -> str:
    return "".join("ACGT"[(w >> (2 * (k - 1 - i))) & 3] for i in range(k))


def revcomp(w: int, k: int) -> int:
    r = 0
    w = ~w & M64
    for _ in range(k):
        r = (r << 2) | (w & 3)
        w >>= 2
    return r


def canonical(w: int, k: int) -> int:
    return min(w, revcomp(w, k))


def revcomp_np(w: np.ndarray, k: int) -> np.ndarray:
    """complement, then the 2-bit groups in reverse order: inside nibbles, inside bytes, the bytes"""
    x = ~np.asarray(w, dtype=np.uint64)
    x = ((x >> np.uint64(2)) & np.uint64(0x3333333333333333)) | ((x & np.uint64(0x3333333333333333)) << np.uint64(2))
    x = ((x >> np.uint64(4)) & np.uint64(0x0F0F0F0F0F0F0F0F)) | ((x & np.uint64(0x0F0F0F0F0F0F0F0F)) << np.uint64(4))
    return x.byteswap() >> np.uint64(64 - 2 * k)


def canonical_np(w: np.ndarray, k: int) -> np.ndarray:
    return np.minimum(w.astype(np.uint64), revcomp_np(w, k))


# ------------------------------------------------------------------ variants

def variant_masks(k: int, n_mm: int, pm_3: int):
    """XOR masks of every variant in the reference's order: the word, then for i = start..k-1, m = 1..3 the subtree
    of mask | m << 2i with start = i + 1 (start = pm_3 at the top)."""
    out = []

    def rec(mask, left, start):
        out.append(mask)
        if not left:
            return
        for i in range(start, k):
            for m in (1, 2, 3):
                rec(mask | (m << (2 * i)), left - 1, i + 1)

    rec(0, n_mm, pm_3)
    return out


def n_variants(k: int, n_mm: int, pm_3: int) -> int:
    from math import comb
    return sum(comb(k - pm_3, c) * 3 ** c for c in range(n_mm + 1))


def masks_np(k: int, n_mm: int, pm_3: int) -> np.ndarray:
    """the same masks as an array (any order is as good for sums): by combinations, without recursion"""
    out = [0]
    for c in range(1, n_mm + 1):
        for pos in itertools.combinations(range(pm_3, k), c):
            for sub in itertools.product((1, 2, 3), repeat=c):
                m = 0
                for p, s in zip(pos, sub):
                    m |= s << (2 * p)
                out.append(m)
    return np.array(out, dtype=np.uint64)


def find_np(keys: np.ndarray, counts: np.ndarray, words: np.ndarray):
    """(present, count or 0) of every word in the sorted key array"""
    if len(keys) == 0:
        return np.zeros(len(words), dtype=bool), np.zeros(len(words), dtype=np.uint32)
    idx = np.searchsorted(keys, words)
    idx[idx == len(keys)] = 0
    hit = keys[idx] == words
    return hit, np.where(hit, counts[idx], 0).astype(np.uint32)


def lookup_np(keys, counts, words, k, n_mm=0, pm_3=0, canonize=True):
    """(values u32, found bool) of gt4hip_query_lookup for an array of query words"""
    words = np.asarray(words, dtype=np.uint64)
    q = canonical_np(words, k) if canonize else words
    if n_mm == 0:
        hit, val = find_np(keys, counts, q)
        return val, hit
    total = np.zeros(len(q), dtype=np.uint64)
    for m in masks_np(k, n_mm, pm_3):
        v = q ^ m
        if canonize:
            v = canonical_np(v, k)
        total += find_np(keys, counts, v)[1]
    val = (total & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return val, val != 0


def lookup_all(keys, counts, word, k, n_mm=0, pm_3=0):
    """[(canonical variant, count)] of one query word in the reference's print order, and the reference's return value"""
    q = canonical(int(word), k)
    table = {int(a): int(b) for a, b in zip(keys, counts)}
    if n_mm == 0:
        return ([(q, table[q])], True) if q in table else ([], False)
    hits, total = [], 0
    for m in variant_masks(k, n_mm, pm_3):
        v = canonical(q ^ m, k)
        if v in table:
            hits.append((v, table[v]))
            total = (total + table[v]) & 0xFFFFFFFF
    return hits, total != 0


def search_one_word(keys, counts, word, k, n_mm=0, pm_3=0, min_freq=0, max_freq=0xFFFFFFFF, print_all=False) -> str:
    """what search_one_word prints for one word"""
    q = canonical(int(word), k)
    hits, found = lookup_all(keys, counts, word, k, n_mm, pm_3)
    if print_all:
        out = "".join("%s\t%u\n" % (word_to_string(v, k), c) for v, c in hits)
        if not found and not min_freq:
            out += "%s\t0\n" % word_to_string(q, k)
        return out
    value = sum(c for _, c in hits) & 0xFFFFFFFF
    if found:
        return "%s\t%u\n" % (word_to_string(q, k), value) if min_freq <= value <= max_freq else ""
    return "%s\t0\n" % word_to_string(q, k) if not min_freq else ""


# ------------------------------------------------------------------ parsers

def fasta_words(text: str, k: int):
    """forward words of a FastA / FastQ text as src/fasta.c:87-300 reads it; (words, return value)"""
    NONE, NAME, SEQ, QUAL = range(4)
    state, fastq, w, n, words = NONE, False, 0, 0, []
    mask = (1 << (2 * k)) - 1
    c2n = {"A": 0, "a": 0, "C": 1, "c": 1, "G": 2, "g": 2, "T": 3, "t": 3, "U": 3, "u": 3}
    i = 0

    def read():
        nonlocal i
        ch = text[i] if i < len(text) else "\0"
        i += 1
        return ch

    while True:
        ch = read()
        if ch == "\0":
            return words, 0
        if state == NONE:
            if ch not in ">@":
                return words, -1
            fastq = ch == "@"
            state = NAME
        elif state == NAME:
            if ch == "\n":
                state, w, n = SEQ, 0, 0
        elif state == SEQ:
            if not fastq and ch == ">":
                state = NAME
            elif fastq and ch == "\n":
                if read() != "+":
                    return words, -1
                ch = read()
                while ch != "\n":
                    if ch == "\0":
                        return words, -1
                    ch = read()
                state = QUAL
            elif ch in c2n:
                w = ((w << 2) | c2n[ch]) & mask
                n = min(n + 1, k)
                if n == k:
                    words.append(w)
            elif ch >= " ":
                w, n = 0, 0
        else:
            if ch == "\n":
                ch = read()
                if ch == "\0":
                    return words, 0
                if ch != "@":
                    return words, -1
                state = NAME


def query_file_words(text: str, k: int, use_3p=False, use_5p=False):
    """words of a -f file as search_n_query_strings reads it (src/glistquery.c:630-659); (words, return value)"""
    words, i, n = [], 0, len(text)

    def cur():
        return ord(text[i]) if i < n else -1

    while cur() > 0:
        line = ""
        while cur() > 0 and len(line) < 255 and text[i] != "\n":
            line += text[i]
            i += 1
        while cur() > 0 and text[i] != "\n":
            i += 1
        while cur() > 0 and cur() < ord("A"):
            i += 1
        if len(line) != k:
            if len(line) < k:
                return words, 1
            if use_3p:
                words.append(string_to_word(line[len(line) - k:], k))
            elif use_5p:
                words.append(string_to_word(line, k))
            else:
                return words, 1
        else:
            words.append(string_to_word(line, k))
    return words, 0


# ------------------------------------------------------------------ statistics

def median_lines(counts: np.ndarray, total: int):
    """(min, max, median as print_median's bisection finds it, average text)"""
    c = np.asarray(counts, dtype=np.uint32)
    n = len(c)
    gmin = int(c.min()) if n else 0xFFFFFFFF
    gmax = int(c.max()) if n else 0
    lo, hi = gmin, gmax
    med = (lo + hi) // 2
    while hi > lo:
        above, below = int((c > med).sum()), int((c < med).sum())
        equal = n - above - below
        if hi == lo + 1:
            if above > below + equal:
                med = hi
            break
        if above > below:
            if above - below < equal:
                break
            lo = med
        elif below > above:
            if below - above < equal:
                break
            hi = med
        else:
            break
        med = ((lo + hi) & 0xFFFFFFFF) // 2
    return gmin, gmax, med


def gc_bases(keys: np.ndarray, counts: np.ndarray, k: int) -> int:
    total = 0
    for w, c in zip(keys, counts):
        w = int(w)
        x = (w ^ (w >> 1)) & 0x5555555555555555 & ((1 << (2 * k)) - 1)
        total += int(c) * bin(x).count("1")
    return total & M64
