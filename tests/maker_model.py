"""glistmaker's reader restated byte by byte in plain Python: fasta_reader_read_nwords (reference src/fasta.c:87-291)
as glistmaker drives it (canonising, src/listmaker-queue.c:196), and the list its words fold into (sort, count: src/word-table.c:217-260;
header of src/word-list.c:33-44).  Slow and obviously right: tests/test_gmaker_model.py holds it to the reference's own
.list files, which licenses it as the expectation for GPU tests on texts that have no golden."""
import numpy as np

from genometester4_amd.listio import header_bytes, make_records

NONE, NAME, SEQUENCE, QUALITY = range(4)
ERR_START, ERR_PLUS, ERR_AT, ERR_PLUS_EOF = 1, 2, 3, 4  # GT4HIP_MAKER_ERR_*

C2N = {}
for _i, _c in enumerate(("Aa", "Cc", "Gg", "TtUu")):
    for _x in _c:
        C2N[ord(_x)] = _i


def read_words(text: bytes, k: int, canonize=True):
    """(words in text order, None | (error kind, offset of the offending byte)); the words are those read before the error"""
    mask = (1 << (2 * k)) - 1
    words = []
    state, fastq = NONE, False
    fw = rv = length = 0
    n = len(text)
    i = 0

    def get(j):
        return text[j] if j < n else 0  # a NUL and the end of the file are the same to the reader

    while True:
        c = get(i)
        if c == 0:
            return words, None
        if state == NONE:
            if c == ord(">"):
                fastq = False
            elif c == ord("@"):
                fastq = True
            else:
                return words, (ERR_START, i)
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
                    return words, (ERR_PLUS, i + 1)
                i += 2
                while get(i) != 10:
                    if get(i) == 0:
                        return words, (ERR_PLUS_EOF, i)
                    i += 1
                state = QUALITY
            elif c in C2N:
                v = C2N[c]
                fw = (fw << 2) | v
                if canonize:
                    rv = (rv >> 2) | ((~v & 3) << ((k - 1) * 2))
                length += 1
                if length > k:
                    fw &= mask
                    length = k
                if length == k:
                    words.append(fw if (not canonize or fw < rv) else rv)
            elif c >= 32:
                fw = rv = length = 0
        else:  # QUALITY
            if c == 10:
                nxt = get(i + 1)
                if nxt == 0:
                    return words, None
                if nxt != ord("@"):
                    return words, (ERR_AT, i + 1)
                i += 1
                state = NAME
        i += 1


def fold(words):
    """(keys ascending, counts) of a sequence of words"""
    keys, counts = np.unique(np.asarray(words, dtype=np.uint64), return_counts=True)
    return keys.astype(np.uint64), counts.astype(np.uint32)


def list_bytes(texts, k):
    """the .list file glistmaker writes for these input files (their words pooled), or None when a reader fails"""
    words = []
    for t in texts:
        w, err = read_words(t, k)
        if err:
            return None
        words += w
    keys, counts = fold(words)
    return header_bytes(k, len(keys), int(counts.sum(dtype=np.uint64)) if len(keys) else 0) + make_records(keys, counts).tobytes()
