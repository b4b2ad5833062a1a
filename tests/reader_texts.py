"""Texts that put the reader's structural bytes on the edges of its geometry (gt4hip_maker.hip, gt4hip_maker_tile.h): a
thread takes P bytes of text, a wavefront W = 64 * P, a tile T = 256 * P, and k_mk_state_scan folds the tiles of a text in
one stretch per thread, of more than one tile only behind SCAN tiles.  The state of the reader at the first byte of each is
rebuilt from carries, and a carry goes wrong where a structural byte is the last byte before or the first byte behind such an
edge.  No GPU here: tests/test_reader_texts_model.py holds these generators to what they promise, tests/test_reader_edges_gpu.py
runs their texts through the library.

  probe (kind)                     one compact well-formed text that holds every structural byte of its format
  sweep (kind, edge, pad_kind)     the probe slid over an edge, once per offset
  hostile (variant, edge)          one changed byte (a missing tag, a NUL) slid over an edge
  grammar (seed, kind)             seeded well-formed texts of one to three tiles from weighted tokens
  units (kind)                     more than SCAN tiles of text whose expectation costs two model calls on 4 kB"""
import os
import re

import numpy as np

import gmer_model
import index_model
import maker_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genometester4_amd", "csrc")
KINDS = ("fasta", "fastq")
K = 5  # the probes hold runs of exactly K - 1, K and K + 1 bases


def _constant(path, pattern):
    m = re.search(pattern, open(os.path.join(CSRC, path)).read())
    assert m, (path, pattern)
    return int(m.group(1))


def geometry():
    """(P, W, T, SCAN): a thread's, a wavefront's and a tile's bytes of text, and the threads of k_mk_state_scan, as the sources say"""
    per = _constant("gt4hip_maker_tile.h", r"constexpr int MK_PER = (\d+);")
    threads = _constant("gt4hip_maker_tile.h", r"constexpr int MK_THREADS = (\d+);")
    wave = _constant("gt4hip_device.h", r"constexpr int WAVE = (\d+);")
    scan = _constant("gt4hip_maker.hip", r"__launch_bounds__ \((\d+)\) void k_mk_state_scan")
    return per, wave * per, threads * per, scan


P, W, T, SCAN = geometry()
EDGES = {"3P": 3 * P, "W": W, "T-W": T - W, "T": T, "2T": 2 * T}
PAD_KINDS = {"fasta": ("name", "sequence"), "fastq": ("name", "sequence", "quality")}

_BASES = bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(20240).integers(0, 4, size=4 * T)])


def bases(n, at=0):
    """n bases, the same ones for the same (n, at)"""
    return (_BASES[at % len(_BASES):] + _BASES * (n // len(_BASES) + 1))[:n]


def cyclic(pattern, n):
    return (pattern * (n // len(pattern) + 1))[:n]


# ------------------------------------------------------------------ probes

_RUNS = b"ACGT"[:K - 1] + b"N" + b"CGTAC"[:K] + b"-" + b"GTACGA"[:K + 1]  # runs of K - 1, K and K + 1 bases
assert len(_RUNS) == 3 * K + 2
_MIXED = b"acguU\x80ACGTA\xffCG*TAn"  # lower case, u / U, bytes of 0x80 and above

FASTA_PROBE = (b">p\n" + _RUNS + b">mid@+>x\n"  # a '>' in mid-line behind bases; the name holds '@', '+', '>' and ends with its '\n'
               + b"GGAT\r\nTC\tAG\x01CT\n"      # "\r\n", a tab and a control byte inside a sequence: the word goes on
               + b">\n>\n"                      # an empty name with an empty sequence, twice
               + _MIXED + b"\n>e\n\nTTGCA\r\n" + bases(36, 7) + b"\n")
FASTQ_PROBE = (b"@p>x@y\n" + _RUNS + b"\n+ACGTNacgt\n@>+II@>+IIIIIIIIII\n"  # the name holds '>' and '@', the '+' line bases; quality begins with '@'
               + b"@q\n\n+\n\n"                                             # an empty sequence with an empty quality line
               + b"@r\nGGAT\rTC\tAG\x01CT" + _MIXED + b"\r\n+\r\n+@IIIIIIIIIIIIIIIIIIIIIIIIIIIII\r\n"
               + b"@\nTTGCA" + bases(36, 7) + b"\n+\n>N>>>\n")              # an empty name
PROBES = {"fasta": FASTA_PROBE, "fastq": FASTQ_PROBE}

# what stands in front of the fill, the fill's pattern, and what closes the record the fill stands in
_PADS = {
    ("fasta", "name"): (b">h", b"ACGTTGCA name ", b"\n"),
    ("fasta", "sequence"): (b">h\n", None, b"\n"),
    ("fastq", "name"): (b"@h", b"ACGTTGCA name ", b"\nACGTA\n+\n@>+II\n"),
    ("fastq", "sequence"): (b"@h\n", None, b"\n+x\n@>+ junk\n"),
    ("fastq", "quality"): (b"@h\nACGTAC\n+\n", b"@>+", b"\n"),
}


def probe(kind):
    return PROBES[kind]


def swept(kind, pad_kind):
    """what a sweep slides over the edge: the bytes that close the pad's record, then the probe"""
    return _PADS[(kind, pad_kind)][2] + PROBES[kind]


def tail(kind, at_least=T + 40):
    """ordinary records"""
    out, i = bytearray(), 0
    while len(out) < at_least:
        if kind == "fasta":
            out += b">t%d\n" % i + b"".join(bases(60, 200 * i + 60 * j) + b"\n" for j in range(3))
        else:
            out += b"@t%d\n" % i + bases(100, 200 * i) + b"\n+\n" + b"I" * 100 + b"\n"
        i += 1
    return bytes(out)


def padded(kind, pad_kind, at, middle, behind):
    """`middle` with its first byte at offset `at`, a pad of `pad_kind` in front of it, `behind` behind it"""
    head, pattern, _ = _PADS[(kind, pad_kind)]
    n = at - len(head)
    assert n >= 0
    return head + (bases(n) if pattern is None else cyclic(pattern, n)) + middle + behind


def sweep_starts(kind, edge, pad_kind, n):
    """where a piece of n bytes starts so that each of its bytes is once the last byte before `edge` and once the first
    behind it (and, one further, the pad's last byte the first behind it); an edge nearer to the start of the text than the
    piece is long is reached by the piece's first bytes only"""
    return range(max(len(_PADS[(kind, pad_kind)][0]), edge - n), edge + 2)


def sweep(kind, edge, pad_kind):
    """(offset of the first swept byte, text) for every offset of the sweep"""
    middle, behind = swept(kind, pad_kind), tail(kind)
    for at in sweep_starts(kind, edge, pad_kind, len(middle)):
        yield at, padded(kind, pad_kind, at, middle, behind)


# ------------------------------------------------------------------ hostile variants

_FQ_REC = b"@b name\nACGTTGCAAC\n+b\nIIIIIIIIII\n"
_FA_REC = b">b name\nACGTTGCAAC\nGGATCCATGA\n"
_FQ_TRAP = b"@t\nACGT\nIIII\n"  # a record without its '+' line: behind a NUL it must not be seen
# variant: (kind, record, offset of the byte in the record, the byte put there, the error kind under the model)
HOSTILE = {
    "no-plus": ("fastq", _FQ_REC, _FQ_REC.index(b"+"), b"x", maker_model.ERR_PLUS),
    "no-at": ("fastq", _FQ_REC, 0, b"x", maker_model.ERR_AT),
    "nul-in-name": ("fastq", _FQ_REC, 3, b"\0", None),
    "nul-in-sequence": ("fastq", _FQ_REC, 12, b"\0", None),
    "nul-in-quality": ("fastq", _FQ_REC, 26, b"\0", None),
    "nul-for-at": ("fastq", _FQ_REC, 0, b"\0", None),
    "nul-behind-sequence-line": ("fastq", _FQ_REC, _FQ_REC.index(b"+"), b"\0", maker_model.ERR_PLUS),
    "nul-in-plus-line": ("fastq", _FQ_REC, _FQ_REC.index(b"+") + 1, b"\0", maker_model.ERR_PLUS_EOF),
    "fasta-nul-in-name": ("fasta", _FA_REC, 3, b"\0", None),
    "fasta-nul-in-sequence": ("fasta", _FA_REC, 12, b"\0", None),
}
HOSTILE_EDGES = ("W", "T", "2T")


def hostile(variant, edge):
    """(offset of the changed byte, text): a good record, the record with the changed byte and (FastQ) a record without
    its '+' line, slid over the edge by a fill inside the first name; ordinary records behind"""
    kind, rec, j, byte, _ = HOSTILE[variant]
    middle = rec + rec[:j] + byte + rec[j + 1:] + (_FQ_TRAP if kind == "fastq" else b"")
    closer = _PADS[(kind, "name")][2]
    behind = tail(kind, 200)
    for at in sweep_starts(kind, edge, "name", len(closer + middle)):
        yield at + len(closer) + len(rec) + j, padded(kind, "name", at, closer + middle, behind)


# ------------------------------------------------------------------ grammar

SEEDS = range(200)
_JUNK = [ord(c) for c in "Nn-*"] + list(range(0x80, 0x100)) + [c for c in range(1, 32) if c != 10]


def line_lengths(k):
    return sorted({0, 1, P - 1, P, P + 1, k - 1, k, k + 1, 60, W - 1, W, W + 1})


def grammar(seed, kind, k=32):
    """a well-formed text of one to three tiles: names empty, short, holding '>' '@' '+' or longer than a tile; lines of the
    lengths line_lengths (k), ended by "\\n" or "\\r\\n", with junk bytes among the bases; FastA with a '>' in mid-line now and
    then; with or without a final newline"""
    rng = np.random.default_rng([seed, KINDS.index(kind)])
    lengths = line_lengths(k)
    weights = np.array([4.0 if n == 60 else 2.0 if k - 1 <= n <= k + 1 else 1.0 for n in lengths])
    fastq = kind == "fastq"
    target = int(rng.integers(T, 3 * T - W))
    had_long = False

    def choice(seq, p=None):
        return seq[int(rng.choice(len(seq), p=None if p is None else np.asarray(p, dtype=float) / sum(p)))]

    def line_end():
        return b"\r\n" if rng.random() < 0.25 else b"\n"

    def name(room):
        nonlocal had_long
        what = choice(["empty", "short", "tags", "long"], [1, 4, 3, 0.0 if had_long or room < T + 4 * W else 0.5])
        if what == "long":
            had_long = True
            return cyclic(b"long name ACGT>@+ ", T + int(rng.integers(1, 2 * W)))
        return {"empty": b"", "short": b"s%d some text" % int(rng.integers(0, 1000)), "tags": b"a>b@c+d ACGT>"}[what]

    def length(room):
        fit = [i for i, n in enumerate(lengths) if n + 2 <= room]
        return lengths[choice(fit, weights[fit])] if fit else 0

    def sequence_line(n):
        s = bytearray(bases(n, int(rng.integers(0, len(_BASES)))))
        if n and rng.random() < 0.2:
            s = bytearray(bytes(s).lower().replace(b"t", b"u" if rng.random() < 0.5 else b"t"))
        if n and rng.random() < 0.4:
            for at in rng.integers(0, n, size=int(rng.integers(1, 4))):
                s[at] = choice(_JUNK + list(b"@+>" if fastq else b"@+"))
        return bytes(s)

    def quality_line(n):
        q = bytearray(cyclic(choice([b"I", b"@>+I", b"#5>"]), n))
        if n and rng.random() < 0.3:
            q[0] = ord("@")
        if n and rng.random() < 0.2:
            q[int(rng.integers(0, n))] = choice([c for c in _JUNK if c != 13])
        return bytes(q)

    def record(room):
        rec = (b"@" if fastq else b">") + name(room) + line_end()
        if fastq:
            rec += sequence_line(length((room - len(rec)) // 2)) + line_end()
            rec += b"+" + choice([b"", b"", b"again", b"ACGTN", b"@>"]) + line_end()
            return rec + quality_line(length(room - len(rec))) + line_end()
        for i in range(int(rng.integers(0, 5))):
            rec += sequence_line(length(room - len(rec) - 2))
            if i < 3 and rng.random() < 0.15:
                return rec  # the next record's '>' stands in mid-line
            rec += line_end()
        return rec

    out = bytearray()
    while len(out) < target and 3 * T - len(out) >= 40:
        rec = record(3 * T - len(out))
        assert len(out) + len(rec) <= 3 * T
        out += rec
    if rng.random() < 0.5 and out.endswith(b"\n"):  # no final newline
        out = out[:-2] if out.endswith(b"\r\n") else out[:-1]
    return bytes(out)


# ------------------------------------------------------------------ units

UNIT = 4099  # coprime to T: the units' starts drift through every offset of a tile
N_UNITS = SCAN + 6


def unit(kind):
    """UNIT bytes that begin with a name and end with a line's '\\n', so no word and no record spans two units"""
    if kind == "fasta":
        body = (b">u1 first\n" + b"".join(bases(60, 60 * j) + b"\n" for j in range(20)) + b">u2>tag\n" + bases(P - 1, 11) + b"\r\n" + bases(70, 5) + b"N" + bases(33, 3)
                + b">mid line\n" + bases(W + 1, 17) + b"\n>\n>u4\n\n" + b"".join(bases(61, 61 * j + 1) + b"\n" for j in range(12)) + b">fill\n")
        body += bases(UNIT - len(body) - 1, 29) + b"\n"
    else:
        body = b"".join(b"@u%d %s\n" % (j, b"a>b@c+"[:j]) + bases(n // 2, 13 * j) + b"Nn"[:n // 99] + bases(n - n // 2, 7 * j) + b"\n+" + b"NACGT"[:j % 3] + b"\n" + cyclic(b"@>+I", n) + b"\n"
                        for j, n in enumerate((100, 0, P + 1, 250, 32, 31, 33, W - 1, 150)))
        body += b"@fill\n"
        n = (UNIT - len(body) - 4) // 2
        body += bases(n, 29) + b"\n+\n" + cyclic(b"I>", UNIT - len(body) - n - 4) + b"\n"
    assert len(body) == UNIT and 0 not in body
    return body


def long_name_unit(kind, at, end=None):
    """a record for offset `at` of a text whose name covers the three whole tiles in front of tile SCAN -- with two tiles to
    a thread of k_mk_state_scan that is one thread's whole stretch, and a border between two stretches -- and ends just
    behind the first byte of tile SCAN; the name holds bases and no '>', so nothing but the carry says "in a name"; the
    sequence is one line that crosses into tile SCAN + 1"""
    if end is None:
        end = SCAN * T + 50
        assert at + 1 <= (SCAN - 3) * T
    rec = (b">" if kind == "fasta" else b"@") + cyclic(b"ACGT tgca ", end - at - 1) + b"\n" + bases(T + 200, 41) + b"\n"
    if kind == "fastq":
        rec += b"+\n" + cyclic(b"@>+I", T + 200) + b"\n"
    return rec


def units(kind, n_units=N_UNITS, a=None, name_end=None):
    """[(text, repeats)]: `a` units, the long-named record, the other units; by default a text of more than SCAN tiles
    (name_end: where the long name ends, for a short text of the same make)"""
    if a is None:
        a = ((SCAN - 3) * T - 1) // UNIT
    u = unit(kind)
    return [(u, a), (long_name_unit(kind, a * UNIT, name_end), 1), (u, n_units - a)]


def units_text(parts):
    return b"".join(t * r for t, r in parts)


def units_cuts():
    """the two cuts of the three-piece case: in mid-name just behind the SCAN-tile mark, and in mid-word one byte before the next tile"""
    return [SCAN * T + 7, (SCAN + 1) * T - 1]


def units_expected(parts, k):
    """what the models give for units_text (parts), from one call per part: dict of words, ordinals, positions, strands
    (uint64 arrays, text order) and subsequences (rows of name_pos, name_len, seq_pos, seq_len)"""
    words, ords, poss, dirs, subs = [], [], [], [], []
    n_seqs = offset = 0
    for text, rep in parts:
        w, o, p, d, s = index_model.read_locations(text, k)
        s = np.array(s, dtype=np.uint64).reshape(-1, 4)
        each = np.arange(rep, dtype=np.uint64)
        words.append(np.tile(np.array(w, dtype=np.uint64), rep))
        ords.append((np.array(o, dtype=np.uint64)[None, :] + (np.uint64(n_seqs) + np.uint64(len(s)) * each)[:, None]).ravel())
        poss.append(np.tile(np.array(p, dtype=np.uint64), rep))
        dirs.append(np.tile(np.array(d, dtype=np.uint64), rep))
        shift = np.repeat(np.uint64(offset) + np.uint64(len(text)) * each, len(s))
        s = np.tile(s, (rep, 1))
        s[:, 0] += shift
        s[:, 2] += shift
        subs.append(s)
        n_seqs += len(s)
        offset += len(text) * rep
    return dict(words=np.concatenate(words), ordinals=np.concatenate(ords), positions=np.concatenate(poss), strands=np.concatenate(dirs),
                subseqs=np.concatenate(subs))


def raw_locations(e):
    """ordinal << 33 | position << 1 | strand of units_expected's arrays"""
    return (e["ordinals"] << np.uint64(33)) | (e["positions"] << np.uint64(1)) | e["strands"]


# ------------------------------------------------------------------ a small database for gmer's counting

def database(text, k=K):
    """every other canonical word of `text` as a gmer_model.Database of one node"""
    words = sorted(set(index_model.read_locations(text, k)[0]))[::2]
    return gmer_model.Database(k, [b"node"], [len(words)], [words])
