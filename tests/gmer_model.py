"""gmer_counter restated in plain Python: the text database (reference src/database.c:20-282), the reader with the
callbacks gmer_counter hangs on it (src/fasta.c:87-291, src/gmer_counter.c:897-936), the counting with its saturation
(:751-815), the statistics and the output (:402-435, :625-711, :945-1005).  Slow and obviously right:
tests/test_gmer_model.py holds it to the reference's own transcripts, which licenses it as the expectation for GPU tests on
inputs that have no golden."""
import os
import re
import struct

VERSION_LINE = "gmer_counter version 4.2.16 (stable)"
USAGE = """Usage:
  gmer_counter ARGUMENTS SEQUENCES...
Arguments:
    -v | --version   - Print version information and exit
    -db DATABASE     - SNP/KMER database file
    -dbb DBBINARY    - binary database file
    -w FILENAME      - write binary database to file
    -32              - use 32-bit integeres for counts (default 16-bit)
    --max_kmers NUM  - maximum number of kmers per node
    --silent         - do not print kmer counts (default for index and binary database compilation)
    --verbose        - print kmer counts (default for counting)
    --header         - print header row
    --total          - print the total number of kmers per node
    --unique         - print the number of nonzero kmers per node
    --kmers          - print individual kmer counts (default if no other output)
    --compile_index FILENAME - Add read index to database and write it to file
    --distribution NUM  - print kmer distribution (up to given number)
    --num_threads    - number of worker threads (default 24)
    --prefetch       - prefetch memory mapped files (faster on high-memory systems)
    --recover        - recover from FastA/FastQ errors (useful for corrupted streams)
    --stats          - print some statistics about sequence and kmers
    -D               - increase debug level
    -DDB             - increase database debug level
"""

C2N = {}
for _i, _c in enumerate(("Aa", "Cc", "Gg", "TtUu")):
    for _x in _c:
        C2N[ord(_x)] = _i

NONE, NAME, SEQUENCE, QUALITY = range(4)


class Refused(Exception):
    """an input the reference misreads and the drop-in refuses with a message of its own"""


def strtol(b: bytes) -> int:
    m = re.match(rb"[ \t\n\v\f\r]*([+-]?[0-9]+)", b)
    return int(m.group(1)) if m else 0


def canonical(w, k):
    r = 0
    x = w
    for _ in range(k):
        r = (r << 2) | (~x & 3)
        x >>= 2
    return min(w, r)


def split_line(c, s, n, max_tokens):
    """split_line, src/utils.c:233-248: [(start, length)]; bytes behind the text read as 0"""
    def at(j):
        return c[j] if j < n else 0
    toks = []
    while len(toks) < max_tokens and at(s) != 10:
        e = s
        while e < n and c[e] >= 32:
            e += 1
        toks.append((s, e - s))
        s = e
        if at(s) != 10:
            s += 1
    return toks


def get_bits(v):
    return v.bit_length()


class Database:
    def __init__(self, wordsize, names, nkmers, words):
        self.wordsize, self.names, self.nkmers, self.words = wordsize, names, nkmers, words  # words: per node, as written
        self.first = []
        at = 0
        for n in nkmers:
            self.first.append(at)
            at += n
        self.n_kmers = at
        self.index = {}  # canonical word -> k-mer index
        for node, ws in enumerate(words):
            for j, w in enumerate(ws):
                c = canonical(w, wordsize)
                if c in self.index:
                    raise Refused("the same canonical k-mer twice")
                self.index[c] = self.first[node] + j


def parse_db(c: bytes, max_kmers_per_node=1000000000):
    """(Database | None, the reference's stderr): gt4_gmer_db_new_from_text"""
    n = len(c)
    if n < 8 or c[5] == 0 or c[7] == 0:
        return None, ""
    if c[n - 1] != 10:
        raise Refused("no final newline")
    # count_lines_from_text, the byte < csize comparison of :68 as it stands
    err = ""
    n_lines = wordsize = max_kmers = 0
    cpos = 0
    while cpos < n:
        if c[cpos] == ord("#"):
            while cpos < n and c[cpos] != 10:
                cpos += 1
            if cpos < n:
                cpos += 1
            continue
        toks = split_line(c, cpos, n, 3)
        if len(toks) < 2:
            err += "Line %u has <2 (%u) tokens\n" % (n_lines, len(toks))
            n_lines = 0
            break
        if not n_lines:
            if len(toks) < 3 or not toks[2][1] or toks[2][1] > 32:
                raise Refused("the first node line gives no word length")
            wordsize = toks[2][1]
        nk = strtol(c[toks[1][0]:]) & 0xffffffff
        max_kmers = max(max_kmers, nk)
        while c[cpos] < n and c[cpos] != 10:
            cpos += 1
        if cpos < n:
            cpos += 1
        n_lines += 1
    if not n_lines:
        return None, err + "File is not text-format kmer database (maybe binary?)\n"
    max_kmers = min(max_kmers, max_kmers_per_node)
    node_bits, kmer_bits = get_bits(n_lines + 1), get_bits(max_kmers)
    if node_bits + kmer_bits > 31:
        return None, err + "Too many nodes and kmers (%u (%u bits), %u (%u bits)\n" % (n_lines + 1, node_bits, max_kmers, kmer_bits)
    # the fill pass, line by line
    names, nkmers, words = [], [], []
    for line in c[:-1].split(b"\n"):
        if line[:1] == b"#":
            continue
        line += b"\n"
        toks = split_line(line, 0, len(line), 3)
        if len(toks) < 2:
            raise Refused("a node line with fewer than 2 tokens")
        nk = strtol(line[toks[1][0]:])
        if nk < 0:
            raise Refused("negative number of k-mers")
        nk = min(nk, max_kmers_per_node)
        ws = []
        cpos = toks[2][0] if len(toks) > 2 else 0
        for _ in range(nk):
            while line[cpos] < 32 and line[cpos] != 10:
                cpos += 1
            if len(toks) < 3 or line[cpos] == 10:
                raise Refused("fewer k-mers than declared")
            w = 0
            for j in range(wordsize):
                if line[cpos + j] not in C2N:
                    raise Refused("a k-mer shorter than the word length or with a character that is no base")
                w = (w << 2) | C2N[line[cpos + j]]
            ws.append(w)
            while line[cpos] >= 32:
                cpos += 1
        names.append(line[toks[0][0]:toks[0][0] + toks[0][1]])
        nkmers.append(nk)
        words.append(ws)
    return Database(wordsize, names, nkmers, words), err


class Reader:
    """fasta_reader_read_nwords with gmer_counter's callbacks: .words (canonical, in text order), .n_n, .n_nucl, .n_gc;
    .error: None | the reference's message line"""

    def __init__(self, text: bytes, k: int, name="x"):
        self.words, self.n_n, self.n_nucl, self.n_gc, self.error = [], 0, 0, 0, None
        mask = (1 << (2 * k)) - 1
        state, fastq = NONE, False
        fw = rv = length = 0
        n = len(text)
        i = 0

        def get(j):
            return text[j] if j < n else 0  # a NUL and the end of the file are the same to the reader

        def fail(msg):
            self.error = "fasta_reader_read_nwords: Reader %s %s\n" % (name, msg)

        while True:
            c = get(i)
            if c == 0:
                return
            if c in (ord("N"), ord("n")):  # read_character: every byte the loop takes
                self.n_n += 1
            if state == NONE:
                if c == ord(">"):
                    fastq = False
                elif c == ord("@"):
                    fastq = True
                else:
                    return fail("invalid start tag '%c'" % c)
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
                        return fail("tag '+' missing, found '%c' instead at %u" % (get(i + 1), i))
                    i += 2
                    while get(i) != 10:
                        if get(i) == 0:
                            return fail("invalid character '%c' after '+' %u" % (0, i))
                        i += 1
                    state = QUALITY
                elif c in C2N:
                    v = C2N[c]
                    self.n_nucl += 1
                    self.n_gc += (v ^ (v >> 1)) & 1
                    fw = (fw << 2) | v
                    rv = (rv >> 2) | ((~v & 3) << ((k - 1) * 2))
                    length += 1
                    if length > k:
                        fw &= mask
                        length = k
                    if length == k:
                        self.words.append(fw if fw < rv else rv)
                elif c >= 32:
                    fw = rv = length = 0
            else:  # QUALITY
                if c == 10:
                    nxt = get(i + 1)
                    if nxt == 0:
                        return
                    if nxt != ord("@"):
                        return fail("tag '@' missing, found '%c' instead at %u" % (nxt, i))
                    i += 1
                    state = NAME
            i += 1


def count(db: Database, texts, names=None):
    """(counts per k-mer, unbounded; stats dict; None | stderr of the first reader error)"""
    counts = [0] * db.n_kmers
    st = dict(n_n=0, n_nucl=0, n_gc=0, n_words=0, n_hits=0, n_kmer_gc=0)
    for t_i, text in enumerate(texts):
        r = Reader(text, db.wordsize, names[t_i] if names else "x")
        if r.error:
            return counts, st, r.error
        st["n_n"] += r.n_n
        st["n_nucl"] += r.n_nucl
        st["n_gc"] += r.n_gc
        st["n_words"] += len(r.words)
        for w in r.words:
            j = db.index.get(w)
            if j is not None:
                counts[j] += 1
                st["n_hits"] += 1
                st["n_kmer_gc"] += db.wordsize * ((w ^ (w >> 1)) & 1)  # (:799-803 reloads the word inside its loop)
    return counts, st, None


def fmt3(num, den):
    if den == 0:
        return "-nan" if num == 0 else "inf"
    return "%.3f" % (num / den)


def pair_median(db, stored, big):
    total, lo, hi = 0, 0xffffffff, 0
    sums = []
    for i in range(len(db.nkmers)):
        total += db.nkmers[i] // 2
        for j in range(0, db.nkmers[i], 2):
            a = db.first[i] + j
            s = stored[a] + (stored[a + 1] if a + 1 < len(stored) else 0)
            if big:
                s &= 0xffffffff
            sums.append(s)
    for s in sums:
        hi, lo = max(hi, s), min(lo, s)
    med = ((lo + hi) & 0xffffffff) // 2
    while hi > lo:
        above = sum(1 for s in sums if s > med)
        below = sum(1 for s in sums if s < med)
        equal = (total - above - below) & 0xffffffff
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
        med = (lo + hi) // 2
    return med


def render(db, counts, st, o, db_name):
    """stdout of a counting run; o: the parsed options"""
    if o["silent"]:
        return b""
    cap = 0xffffffff if o["big"] else 65535
    stored = [min(c, cap) for c in counts]
    # what --unique reads: the counters' bytes as 16-bit words (with -32 too, src/gmer_counter.c:655-659)
    halves = stored if not o["big"] else list(struct.unpack("<%dH" % (2 * len(stored)), struct.pack("<%dI" % len(stored), *stored)))
    out = ["#" + VERSION_LINE + "\n", "#TextDatabase\t%s\n" % db_name]
    if o["dm"]:
        out.append("#PairMedian\t%u\n" % pair_median(db, stored, o["big"]))
    if o["stats"]:
        out.append("#LENGTH\t%u\n" % (st["n_nucl"] + st["n_n"]))
        out.append("#LENGTH_ACGT\t%u\n" % st["n_nucl"])
        out.append("#GC\t%s\n" % fmt3(st["n_gc"], st["n_nucl"]))
        out.append("#TOTAL_KMERS\t%u\n" % st["n_words"])
        out.append("#LIST_KMERS\t%u\n" % st["n_hits"])
        out.append("#LIST_KMER_GC\t%s\n" % fmt3(st["n_kmer_gc"], st["n_hits"] * db.wordsize))
    if o["header"]:
        out.append("NODE\tN_KMERS" + ("\tTOTAL" if o["total"] else "") + ("\tUNIQUE" if o["unique"] else "") + ("\tKMERS" if o["kmers"] else "") +
                   ("\tDISTRIBUTION" if o["distro"] else "") + "\n")
    res = ["".join(out).encode("latin-1")]
    for i, name in enumerate(db.names):
        nk, first = db.nkmers[i], db.first[i]
        mine = stored[first:first + nk]
        row = [name, b"\t%d" % nk]
        if o["total"]:
            row.append(b"\t%d" % sum(mine))
        if o["unique"]:
            row.append(b"\t%d" % sum(1 for h in halves[first:first + nk] if h))
        if o["kmers"]:
            row += [b"\t%d" % c for c in mine]
        if o["distro"]:
            srt = sorted(mine)
            j = 0
            cols = []
            for current in range(o["distro"] + 1):
                cnt = 0
                while j < nk and srt[j] == current:
                    cnt += 1
                    j += 1
                cols.append(b"\t%d" % cnt)
            row.append(b"".join(cols))
        row.append(b"\n")
        res.append(b"".join(row))
    return b"".join(res)


def parse_argv(argv):
    """(options, None) | (None, (exit, stdout, stderr)): main, :155-282"""
    o = dict(db=None, dbb=None, wdb=None, index=None, max_kmers=1000000000, silent=0, big=0, dm=0, header=0, total=0, unique=0, kmers=0,
             distro=0, stats=0, recover=0, files=[], refused=None)
    usage = VERSION_LINE + "\n" + USAGE
    i = 0

    def value():
        nonlocal i
        i += 1
        return argv[i] if i < len(argv) else None

    valued = {"-db": "db", "-dbb": "dbb", "-w": "wdb", "--compile_index": "index"}
    while i < len(argv):
        a = argv[i]
        if a in ("-v", "--version"):
            return None, (0, VERSION_LINE + "\n", "")
        if a in ("-h", "--help"):
            return None, (0, usage, "")
        if a in valued or a in ("--max_kmers", "--distribution", "--num_threads"):
            v = value()
            if v is None:
                return None, (1, "", usage)
            if a in valued:
                o[valued[a]] = v
                if a != "-db" and not o["refused"]:
                    o["refused"] = a
            elif a == "--max_kmers":
                o["max_kmers"] = strtol(v.encode()) & 0xffffffff
            elif a == "--distribution":
                o["distro"] = strtol(v.encode()) & 0xffffffff
        elif a in ("--silent", "--header", "--total", "--unique", "--kmers", "--recover"):
            o[a[2:]] = 1
        elif a == "-32":
            o["big"] = 1
        elif a == "--double_median":
            o["dm"] = 1
        elif a in ("--stats", "-stat"):
            o["stats"] = 1
        elif a in ("--export_reads", "--count_trie_allocations", "--dump_index"):
            o["refused"] = o["refused"] or a
        elif a in ("--verbose", "--prefetch", "-D", "-DDB"):
            pass
        else:
            o["files"].append(a)
        i += 1
    if not o["files"] and not o["wdb"]:
        return None, (1, "", "Nothing to do!\n" + usage)
    if o["db"] and o["dbb"]:
        return None, (1, "", "Both text and binary database specifed\n" + usage)
    if o["dbb"] and o["wdb"]:
        return None, (1, "", "Binary database read and written\n" + usage)
    if not o["total"] and not o["unique"] and not o["distro"]:
        o["kmers"] = 1
    o["distro"] = min(o["distro"], 65536)
    return o, None


def run(argv, read_file):
    """(exit, stdout bytes, stderr str) of `gmer_counter argv`; read_file (name) -> bytes | None.  Raises Refused where
    the drop-in refuses what the reference misreads."""
    o, done = parse_argv(argv)
    if done:
        return done[0], done[1].encode(), done[2]
    if o["refused"] or not o["db"] or "-" in o["files"]:
        raise Refused("an option or input this program does not take")
    text = read_file(o["db"])
    if text is None:
        return 1, b"", "gt4_mmap (stat): %s\nCannot mmap database file %s\n" % (os.strerror(2), o["db"])
    if not text:
        return 1, b"", "gt4_mmap (mmap): %s\nCannot mmap database file %s\n" % (os.strerror(22), o["db"])
    db, err = parse_db(text, o["max_kmers"])
    if db is None:
        return 1, b"", err + "Cannot read text database (null)\n"
    texts = []
    for f in o["files"]:
        t = read_file(f)
        if t is None:
            return 1, b"", "fasta_reader_read_nwords: Reader %s read error (-1) at 0\nread_file: Fasta reader %s returned 4294967295\n" % (f, f)
        texts.append(t)
    counts, st, rerr = count(db, texts, o["files"])
    if rerr:
        name = rerr.split("Reader ")[1].split(" ")[0]
        return 1, b"", rerr + "read_file: Fasta reader %s returned 4294967295\n" % name
    return 0, render(db, counts, st, o, o["db"]), ""
