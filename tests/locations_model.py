"""A Python restatement of what the reference's glistquery does with a GT4I index (reference src/glistquery.c:439-568,
:702-717; src/index-map.c:123-314): the parse of the file, --files, --sequences, the dump with --locations, and the
query forms with their locations and the sticky REVERSE flag.  Lookups are by enumeration (tests/query_model.py).
Nothing here touches a device; the GPU tests and the command line are held to it."""
import os
import struct

import numpy as np

import gquery_util as U
import query_model as M

HEADER = struct.Struct("<4I2Q4I3Q")
INDEX_CODE = 0x47543449
LIST_CODE = 0x47543443


class Index:
    """a GT4I file taken apart"""

    def __init__(self, data: bytes):
        (code, self.major, self.minor, self.k, n, self.n_locations, fb, sb, pb, _, f_at, k_at, l_at) = HEADER.unpack_from(data, 0)
        assert code == INDEX_CODE
        self.bits = (fb, sb, pb)
        self.kmers = np.frombuffer(data, dtype="<u8", count=2 * n, offset=k_at).reshape(-1, 2)
        self.locations = np.frombuffer(data, dtype="<u8", count=self.n_locations, offset=l_at)
        self.words = self.kmers[:, 0]
        first = np.append(self.kmers[:, 1], np.uint64(self.n_locations))
        self.first = first[:-1]
        self.counts = (first[1:] - first[:-1]).astype(np.uint32)  # imap_get_count: 32 bits
        self.files = []
        if f_at + 16 <= len(data):
            at = f_at + 16
            for _ in range(struct.unpack_from("<I", data, f_at + 12)[0]):
                size, n_seq, ln = struct.unpack_from("<QQH", data, at)
                name = data[at + 18:at + 18 + ln].split(b"\0")[0].decode("latin-1")
                at += 18 + ln
                seqs = [struct.unpack_from("<QIQQ", data, at + 28 * j) for j in range(n_seq)]  # name_pos, name_len, seq_pos, seq_len
                at += 28 * n_seq
                self.files.append((size, n_seq, name, seqs))

    def decode(self, code):
        """(file, sequence, position, strand) of a packed location (index_map_get_location)"""
        fb, sb, pb = self.bits
        code = int(code)

        def field(shift, bits):
            return (code >> shift) & ((1 << bits) - 1) if shift < 64 else 0

        return field(sb + pb + 1, fb) & 0xFFFFFFFF, field(pb + 1, sb) & 0xFFFFFFFF, field(1, pb), code & 1

    def places(self, i):
        """the decoded locations of word number i"""
        a = int(self.first[i])
        return [self.decode(c) for c in self.locations[a:a + int(self.counts[i])]]


def location_lines(places, reverse=0):
    return "".join("%u\t%u\t%u\t%u\n" % (f, s, p, d ^ reverse) for f, s, p, d in places)


def print_files(ix: Index) -> str:
    return "".join("%u\t%s\t%u\t%u\n" % (i, name, size, n) for i, (size, n, name, _) in enumerate(ix.files))


def print_sequences(ix: Index, cwd: str):
    """(stdout, names of the sources that could not be mapped, once per sequence as the reference complains)"""
    out, missing = [], []
    for i, (_, _, fname, seqs) in enumerate(ix.files):
        try:
            src = open(os.path.join(cwd, fname), "rb").read()
        except OSError:
            src = None
        for j, (name_pos, name_len, seq_pos, seq_len) in enumerate(seqs):
            if src is None:
                missing.append(fname)
                name = b""
            else:
                name = src[name_pos:name_pos + min(name_len, 1023)].split(b"\0")[0]
            out.append("%u\t%u\t%s\t%u\t%u\t%u\n" % (i, j, name.decode("latin-1"), name_pos, seq_pos, seq_len))
    return "".join(out), missing


def dump(ix: Index, locations: bool) -> str:
    out = []
    for i in range(len(ix.words)):
        out.append("%s\t%u\n" % (M.word_to_string(int(ix.words[i]), ix.k), ix.counts[i]))
        if locations:
            out.append(location_lines(ix.places(i)))
    return "".join(out)


class Searcher:
    """search_one_word with an index and --locations: REVERSE rises with the first query whose reverse complement is the
    smaller word and never falls"""

    def __init__(self, ix: Index, n_mm=0, pm_3=0, min_freq=0, max_freq=0xFFFFFFFF, print_all=False):
        self.ix, self.n_mm, self.pm_3, self.min_freq, self.max_freq, self.print_all = ix, n_mm, pm_3, min_freq, max_freq, print_all
        self.reverse = 0
        self.where = {int(w): i for i, w in enumerate(ix.words.tolist())}
        self.masks = M.variant_masks(ix.k, n_mm, pm_3) if n_mm else [0]

    def lookup_all(self, q: int):
        """query_model.lookup_all over the index's words, the table kept: ([(canonical variant, count)] in the reference's
        order, its return value)"""
        k, hits, total = self.ix.k, [], 0
        for m in self.masks:
            v = M.canonical(q ^ m, k) if self.n_mm else q
            i = self.where.get(v)
            if i is not None:
                hits.append((v, int(self.ix.counts[i])))
                total = (total + hits[-1][1]) & 0xFFFFFFFF
        return hits, (total != 0 if self.n_mm else bool(hits))

    def search_plain(self, word: int) -> str:
        """without --locations: query_model.search_one_word"""
        k = self.ix.k
        q = M.canonical(int(word), k)
        hits, found = self.lookup_all(q)
        if self.print_all:
            return "".join("%s\t%u\n" % (M.word_to_string(v, k), c) for v, c in hits) + ("%s\t0\n" % M.word_to_string(q, k) if not found and not self.min_freq else "")
        value = sum(c for _, c in hits) & 0xFFFFFFFF
        if found:
            return "%s\t%u\n" % (M.word_to_string(q, k), value) if self.min_freq <= value <= self.max_freq else ""
        return "%s\t0\n" % M.word_to_string(q, k) if not self.min_freq else ""

    def search(self, word: int) -> str:
        k = self.ix.k
        q = M.canonical(int(word), k)
        if q != int(word):
            self.reverse = 1
        hits, found = self.lookup_all(q)
        out = []
        for w, c in hits:
            out.append("%s\t%u\t%u\n" % (M.word_to_string(w, k), c, self.reverse))
            out.append(location_lines(self.ix.places(self.where[w]), self.reverse))
        if not found and not self.min_freq:
            out.append("%s\t0\n" % M.word_to_string(q, k))
        return "".join(out)


def zipper(ix: Index, q_words, q_counts, locations: bool) -> str:
    """-l without mismatches: the QUERY list's count, REVERSE 0, the index's locations"""
    where = {int(w): i for i, w in enumerate(ix.words)}
    out = []
    for w, c in zip(q_words, q_counts):
        if int(w) in where:
            out.append("%s\t%u%s\n" % (M.word_to_string(int(w), ix.k), c, "\t0" if locations else ""))
            if locations:
                out.append(location_lines(ix.places(where[int(w)])))
    return "".join(out)


def read_list(data: bytes):
    """(k, words, counts) of a .list file"""
    k, n = struct.unpack_from("<I", data, 12)[0], struct.unpack_from("<Q", data, 16)[0]
    start = struct.unpack_from("<Q", data, 32)[0]
    rec = np.frombuffer(data, dtype=np.dtype([("w", "<u8"), ("c", "<u4")]), count=n, offset=start)
    return k, rec["w"], rec["c"]


def replay(argv, cwd):
    """(stdout, exit code) of `glistquery argv` run in cwd, for the forms of tests/golden/gqloc_cases.json"""
    p = U.parse(argv)
    locations = "--locations" in p["other"]
    blobs = [open(os.path.join(cwd, n), "rb").read() for n in p["lists"]]
    is_index = [struct.unpack_from("<I", b, 0)[0] == INDEX_CODE for b in blobs]
    for opt in ("--files", "--sequences"):
        if opt in p["other"]:
            if len(blobs) != 1 or not is_index[0]:
                return "", 1
            ix = Index(blobs[0])
            return (print_files(ix) if opt == "--files" else print_sequences(ix, cwd)[0]), 0
    assert len(blobs) == 1 and is_index[0], argv
    ix = Index(blobs[0])
    k = ix.k
    if p["l"] is not None:
        q = open(os.path.join(cwd, p["l"]), "rb").read()
        if struct.unpack_from("<I", q, 0)[0] != LIST_CODE:
            return "", 1  # the query list is streamed: a .list only
        _, q_words, q_counts = read_list(q)
        if not p["mm"]:
            return zipper(ix, q_words, q_counts, locations), 0
        words, rc = [int(w) for w in q_words], 0
    elif p["q"] is not None:
        words, rc = M.query_file_words(p["q"] + "\n", k, p["use_3p"], p["use_5p"])
    elif p["f"] is not None:
        words, rc = M.query_file_words(open(os.path.join(cwd, p["f"]), "rb").read().decode("latin-1"), k, p["use_3p"], p["use_5p"])
    elif p["s"] is not None:
        words, rc = M.fasta_words(open(os.path.join(cwd, p["s"]), "rb").read().decode("latin-1"), k)
    else:
        return dump(ix, locations), 0
    s = Searcher(ix, p["mm"], p["p"], p["min"], p["max"], p["all"])
    return "".join(s.search(w) if locations else s.search_plain(w) for w in words), rc & 0xFF
