"""glistquery --mask restated on the CPU, byte by byte: the reader of tests/maker_model.py (the same state machine, which
here also remembers where every base stands) and the lookup rule of tests/query_model.py as tests/seqprofile_model.py
applies it.  Slow and obviously right: tests/test_gqmask_model.py holds it to tests/golden/gqmask_cases.json, which was
derived from the reference's own `glistquery -s`; that licenses it as the expectation of the GPU tests."""
import numpy as np

import maker_model
import seqprofile_model
from maker_model import C2N, ERR_AT, ERR_PLUS, ERR_PLUS_EOF, ERR_START, NAME, NONE, QUALITY, SEQUENCE


def read_bases(text: bytes, k: int):
    """(words in text order, for each word the index of its LAST base in `bases`, bases: the offset of every base byte of a
    sequence line in text order, None | (error kind, offset)).  The k bases of word i are bases[last[i] - k + 1 .. last[i]]:
    a run's bases are neighbours in `bases`, whatever bytes < ' ' lie between them in the text."""
    mask = (1 << (2 * k)) - 1
    words, last, bases = [], [], []
    state, fastq = NONE, False
    fw = rv = length = 0
    n = len(text)
    i = 0

    def get(j):
        return text[j] if j < n else 0

    def done(err):
        return words, last, bases, err

    while True:
        c = get(i)
        if c == 0:
            return done(None)
        if state == NONE:
            if c == ord(">"):
                fastq = False
            elif c == ord("@"):
                fastq = True
            else:
                return done((ERR_START, i))
            state = NAME
        elif state == NAME:
            if c == 10:
                state = SEQUENCE
                fw = rv = length = 0
        elif state == SEQUENCE:
            if not fastq and c == ord(">"):
                state = NAME
            elif fastq and c == 10:
                if get(i + 1) != ord("+"):
                    return done((ERR_PLUS, i + 1))
                i += 2
                while get(i) != 10:
                    if get(i) == 0:
                        return done((ERR_PLUS_EOF, i))
                    i += 1
                state = QUALITY
            elif c in C2N:
                v = C2N[c]
                fw = (fw << 2) | v
                rv = (rv >> 2) | ((~v & 3) << ((k - 1) * 2))
                length += 1
                bases.append(i)
                if length > k:
                    fw &= mask
                    length = k
                if length == k:
                    words.append(fw if fw < rv else rv)
                    last.append(len(bases) - 1)
            elif c >= 32:
                fw = rv = length = 0
        else:  # QUALITY
            if c == 10:
                nxt = get(i + 1)
                if nxt == 0:
                    return done(None)
                if nxt != ord("@"):
                    return done((ERR_AT, i + 1))
                i += 1
                state = NAME
        i += 1


class Masked:
    """what mask_text gives: the masked text, (n_words, n_hits, n_covered), the reader's error, and per word / per base what
    backs () needs"""

    def __init__(self, text, counts, err, last, bases, hit, covered, k):
        self.text, self.counts, self.err = text, counts, err
        self.last, self.bases, self.hit, self.covered, self.k = last, bases, hit, covered, k

    def own_covered(self, cuts):
        """n_covered of every piece of the text cut at `cuts`: the piece's bases inside a hit word that ENDS in the piece"""
        edges = [0] + list(cuts) + [len(self.text)]
        end = self.bases[self.last] if len(self.last) else np.zeros(0, dtype=np.int64)
        out = []
        for s, e in zip(edges[:-1], edges[1:]):
            sel = self.hit & (end >= s) & (end < e)
            d = np.zeros(len(self.bases) + 1, dtype=np.int64)
            np.add.at(d, self.last[sel] - (self.k - 1), 1)
            np.add.at(d, self.last[sel] + 1, -1)
            out.append(int(((np.cumsum(d)[:-1] > 0) & (self.bases >= s) & (self.bases < e)).sum()))
        return out

    def own_text(self, cuts, source: bytes, soft=False, mask_byte=b"N") -> bytes:
        """the pieces as gt4hip_query_mask_text gives them, one after the other: in every piece of `source` (the text
        before masking) only the bases inside a hit word that ENDS in the piece are replaced"""
        edges = [0] + list(cuts) + [len(self.text)]
        end = self.bases[self.last] if len(self.last) else np.zeros(0, dtype=np.int64)
        out = bytearray(source)
        for s, e in zip(edges[:-1], edges[1:]):
            for w in np.flatnonzero(self.hit & (end >= s) & (end < e)).tolist():
                for p in self.bases[self.last[w] - self.k + 1:self.last[w] + 1].tolist():
                    if p >= s:
                        out[p] = (source[p] | 0x20) if soft else mask_byte[0]
        return bytes(out)

    def backs(self, cuts):
        """`back` of every piece of the text cut at the offsets `cuts` (ascending; pieces [0, cuts[0]), [cuts[0], cuts[1]),
        ..., [cuts[-1], end)): the most bases in front of the piece that a hit word ending in the piece holds"""
        edges = [0] + list(cuts) + [len(self.text)]
        out = []
        first = self.bases[self.last - (self.k - 1)] if len(self.last) else np.zeros(0, dtype=np.int64)
        end = self.bases[self.last] if len(self.last) else np.zeros(0, dtype=np.int64)
        for s, e in zip(edges[:-1], edges[1:]):
            best = 0
            for w in np.flatnonzero(self.hit & (end >= s) & (end < e) & (first < s)).tolist():
                word_bases = self.bases[self.last[w] - self.k + 1:self.last[w] + 1]
                best = max(best, int((word_bases < s).sum()))
            out.append(best)
        return out


def mask_text(keys, counts, text: bytes, k, n_mm=0, pm_3=0, lo=1, hi=0xFFFFFFFF, soft=False, mask_byte=b"N") -> Masked:
    """The text with every base inside a hit word replaced (mask_byte, or byte | 0x20 when soft); a word is a hit when it is
    found and lo <= value <= hi (seqprofile_model.hits_np).  After a reader error the words in front of it count."""
    words, last, bases, err = read_bases(text, k)
    assert words == maker_model.read_words(text, k)[0]
    last, bases = np.array(last, dtype=np.int64), np.array(bases, dtype=np.int64)
    covered = np.zeros(len(bases), dtype=bool)
    hit = np.zeros(len(words), dtype=bool)
    if words:
        hit, _ = seqprofile_model.hits_np(keys, counts, np.array(words, dtype=np.uint64), k, n_mm, pm_3, lo, hi)
        d = np.zeros(len(bases) + 1, dtype=np.int64)
        np.add.at(d, last[hit] - (k - 1), 1)
        np.add.at(d, last[hit] + 1, -1)
        covered = np.cumsum(d)[:-1] > 0
    out = bytearray(text)
    for p in bases[covered].tolist():
        out[p] = (out[p] | 0x20) if soft else mask_byte[0]
    return Masked(bytes(out), (len(words), int(hit.sum()), int(covered.sum())), err, last, bases, hit, covered, k)
