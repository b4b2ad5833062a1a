"""glistmaker --index restated byte by byte in plain Python: the reader of tests/maker_model.py with the callbacks the
reference hangs on it for an index (start_sequence_index, end_sequence_index, read_word_index: reference
src/glistmaker.c:1031-1067 on src/fasta.c:87-291) and the writer of the GT4I file (write_index, :366-782).  Slow and
obviously right: tests/test_gindex_model.py holds it to the reference's own .index files, which licenses it as the
expectation for GPU tests.

Not modelled: files the reference cuts into blocks (above 10^8 bytes, src/listmaker-queue.c:28) and what it leaves
behind after a reader error."""
import struct

import numpy as np

from maker_model import C2N

NONE, NAME, SEQUENCE, QUALITY = range(4)
MASKED = (6, 7, 10, 11)  # bytes of the file block that the reference writes from behind a 2-byte variable (:380-389)


def read_locations(text: bytes, k: int):
    """(words, ordinals, positions, strands, subsequences) of one file; words in text order, the ordinal of a word is the
    index of its subsequence, a subsequence is [name_pos, name_len, seq_pos, seq_len] in bytes of the file"""
    mask = (1 << (2 * k)) - 1
    words, ords, poss, dirs, subs = [], [], [], [], []
    state, fastq = NONE, False
    fw = rv = length = 0
    npos = name_pos = name_len = 0
    n = len(text)
    i = 0  # the reader's cpos is the offset of the byte in hand throughout

    def get(j):
        return text[j] if j < n else 0

    def new_name(tag_at):
        nonlocal state, npos, name_pos, name_len
        state, npos, name_pos, name_len = NAME, 0, tag_at + 1, 0

    while True:
        c = get(i)
        if c == 0:
            if state == SEQUENCE:
                subs[-1][3] = i - subs[-1][2]
            break
        if state == NONE:
            assert c in (ord(">"), ord("@")), "not modelled: reader errors"
            fastq = c == ord("@")
            new_name(i)
        elif state == NAME:
            if c == 10:
                state = SEQUENCE
                fw = rv = length = 0
                subs.append([name_pos, name_len, i + 1, 0])
            else:
                name_len += 1
        elif state == SEQUENCE:
            if not fastq and c == ord(">"):
                subs[-1][3] = i - subs[-1][2]
                new_name(i)
            elif fastq and c == 10:
                subs[-1][3] = i - subs[-1][2]
                assert get(i + 1) == ord("+"), "not modelled: reader errors"
                i += 2
                while get(i) != 10:
                    assert get(i) != 0, "not modelled: reader errors"
                    i += 1
                state = QUALITY
            elif c in C2N:
                v = C2N[c]
                fw = (fw << 2) | v
                rv = (rv >> 2) | ((~v & 3) << ((k - 1) * 2))
                length += 1
                if length > k:
                    fw &= mask
                    length = k
                if length == k:
                    w = fw if fw < rv else rv
                    words.append(w)
                    ords.append(len(subs) - 1)
                    poss.append(npos + 1 - k)
                    dirs.append(int(w != fw))
                npos += 1
            elif c >= 32:
                fw = rv = length = 0
                npos += 1
        else:  # QUALITY
            if c == 10:
                nxt = get(i + 1)
                if nxt == 0:
                    break
                assert nxt == ord("@"), "not modelled: reader errors"
                i += 1
                new_name(i)
        i += 1
    return words, ords, poss, dirs, subs


def bitsize(v):
    """get_bitsize (:116-126)"""
    return max(1, int(v).bit_length())


def pairs(texts, k):
    """every word of the files with its packed location, in text order, and what the file block needs:
    (words, locations, (file bits, subsequence bits, position bits), subsequences per file)"""
    per_file = [read_locations(t, k) for t in texts]
    max_sub = max([len(f[4]) - 1 for f in per_file if f[4]] + [0])
    max_pos = max([max(f[2]) for f in per_file if f[0]] + [0])
    fb, sb, pb = bitsize(len(texts) - 1), bitsize(max_sub), bitsize(max_pos)
    words, locs = [], []
    for fi, (w, o, p, d, _) in enumerate(per_file):
        words += w
        locs += [(fi << (sb + pb + 1)) | (oo << (pb + 1)) | (pp << 1) | dd for oo, pp, dd in zip(o, p, d)]
    return words, locs, (fb, sb, pb), [f[4] for f in per_file]


def sections(words, locs, lo=1, hi=0xffffffff):
    """write_kmers + write_locations (:425-574): ((word, first location) of the words the cut-offs keep, n_locations, every
    location sorted by word and ascending within a word)"""
    w = np.asarray(words, dtype=np.uint64)
    v = np.asarray(locs, dtype=np.uint64)
    order = np.lexsort((v, w))
    kmers, at = [], 0
    keys, counts = np.unique(w, return_counts=True)
    for key, c in zip(keys.tolist(), counts.tolist()):
        if lo <= c <= hi:
            kmers.append((key, at))
            at += c
    return kmers, at, v[order]


def index_bytes(texts, names, k, lo=1, hi=0xffffffff, table=sections):
    """the .index file glistmaker --index writes for these files (names as given on the command line); `table`: what
    makes the two sections of the pairs (the GPU tests put the library's table step here)"""
    words, locs, (fb, sb, pb), subs = pairs(texts, k)
    if not words:  # write_index_header (:576-626)
        return b"I4TG" + struct.pack("<3I2Q4I3Q", 4, 2, k, 0, 0, 1, 1, 1, 0, 72, 72, 72)
    kmers, n_locs, sorted_locs = table(words, locs, lo, hi)
    block = b"F4TG" + struct.pack("<3I", 4, 2, len(texts))
    for t, name, ss in zip(texts, names, subs):
        nm = name.encode("latin-1") + b"\0"
        block += struct.pack("<QQH", len(t), len(ss), len(nm)) + nm
        for s in ss:
            block += struct.pack("<QIQQ", *s)
    block += b"\0" * (-len(block) % 8)
    km = np.asarray(kmers, dtype=np.uint64).reshape(-1, 2).tobytes()
    head = b"I4TG" + struct.pack("<3I2Q4I3Q", 4, 2, k, len(kmers), int(n_locs), fb, sb, pb, 0, 72, 72 + len(block), 72 + len(block) + len(km))
    return head + block + km + np.asarray(sorted_locs, dtype=np.uint64).tobytes()


def masked(data: bytes):
    """an index file with the four undefined bytes of its file block zeroed"""
    b = bytearray(data)
    if len(b) > 72:
        at = struct.unpack_from("<Q", b, 48)[0]
        for j in MASKED:
            b[at + j] = 0
    return bytes(b)


def parse(data: bytes):
    """header fields and the two arrays of an index file"""
    major, minor, k, n_kmers, n_locs, fb, sb, pb, _, f_at, k_at, l_at = struct.unpack_from("<3I2Q4I3Q", data, 4)
    kmers = np.frombuffer(data, dtype=np.uint64, count=2 * n_kmers, offset=k_at).reshape(-1, 2)
    locs = np.frombuffer(data, dtype=np.uint64, offset=l_at)
    return dict(k=k, n_kmers=n_kmers, n_locations=n_locs, bits=(fb, sb, pb), kmers=kmers, locations=locs)
