#!/usr/bin/env python3
"""Golden transcripts of the reference's glistquery for the forms genometester4_amd/glistquery reproduces on the
device: the statistics commands, the dump of one list, -q / -f / -s / -l with -mm, -p, -min, -max, --all, --3p, --5p,
and every early error (reference src/glistquery.c:108-437).

Needs oracle/_ref/glistquery (make -C oracle ref).  Writes tests/golden/gquery_cases.json:

    inputs   names of lists taken from inputs.npz
    lists    {name: [zlib + base64 of the packed 12-byte records, word length]}: small lists made here (data only)
    files    {name: text}: query, FastA and FastQ files (latin-1)
    cases    [{id, argv, exit, stdout | (stdout_sha256, stdout_bytes, stdout_head), stderr (where deterministic)}]

A long stdout is recorded as its SHA-256, its length and its first bytes, which pins every byte all the same."""
import base64
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from genometester4_amd.listio import RECORD_DTYPE, make_records, write_list  # noqa: E402
import query_model as M  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "glistquery")
FULL_STDOUT = 3000  # bytes kept verbatim


def word(s):
    return M.string_to_word(s, len(s))


def canon_list(words, k, counts):
    w = np.unique(np.array([M.canonical(int(x), k) for x in words], dtype=np.uint64))
    return make_records(w, np.asarray(counts, dtype=np.uint32)[:len(w)])


def seq(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, size=n))


def mutate(rng, s, n):
    s = list(s)
    for p in rng.choice(len(s), size=n, replace=False):
        s[p] = "ACGT"[("ACGT".index(s[p]) + int(rng.integers(1, 4))) % 4]
    return "".join(s)


def main():
    if not os.path.exists(REF):
        sys.exit("build the reference first: make -C oracle ref")
    t0 = time.time()
    rng = np.random.default_rng(77)
    inp = np.load(os.path.join(HERE, "inputs.npz"))
    meta = json.loads(bytes(inp["__meta__"]).decode())
    work = tempfile.mkdtemp(prefix="gt4gquery_")
    inputs = ["A8", "B8", "H1", "H2", "R1", "R2", "W1", "E8", "K9", "M0", "M1"]
    for n in inputs:
        write_list(os.path.join(work, n + ".list"), inp[n].astype(RECORD_DTYPE), meta[n][0])
    lists, files = {}, {}

    def add_list(name, rec, k):
        lists[name] = (rec, k)
        write_list(os.path.join(work, name + ".list"), rec, k)

    def add_file(name, text):
        files[name] = text
        with open(os.path.join(work, name), "wb") as f:
            f.write(text.encode("latin-1"))

    # k = 4: most of the canonical 4-mers
    all4 = sorted({M.canonical(w, 4) for w in range(256)})
    k4 = np.unique(np.array(all4[::2] + all4[1::7], dtype=np.uint64))
    add_list("K4", make_records(k4, rng.integers(1, 50, size=len(k4))), 4)

    # k = 16: random words; one query word Q16 with neighbours at depth 0, 1 and 2 in the list
    q16 = "CCAGAAAATAGCGACG"
    base16 = [seq(rng, 16) for _ in range(300)]
    d1 = [q16[:3] + "T" + q16[4:], q16[:15] + "A"]
    d2 = [q16[:3] + "T" + q16[4:9] + "C" + q16[10:], "G" + q16[1:14] + "TG"]
    add_list("L16", canon_list([word(s) for s in base16 + [q16] + d1 + d2], 16, rng.integers(1, 9, size=400)), 16)
    # the reverse-palindromic query ACGTACGTACGTACGT and its neighbour: looked up twice
    add_list("P16", make_records([word("ACGTACGTACGTACGA")], [1]), 16)
    # stored counts of 0: found at -mm 0, nothing at -mm 1
    z16 = [M.canonical(word(s), 16) for s in ("AAAACCCCGGGGTTTA", "AAAACCCCGGGGTTCA", "ACACACACACACAGAG")]
    add_list("Z16", make_records(np.sort(np.array(z16, dtype=np.uint64)), [0, 0, 0]), 16)
    # counts whose sum passes 2^32
    big = "AACCGGTTAACCGGTA"
    bw = np.unique(np.array([M.canonical(word(s), 16) for s in (big, big[:5] + "A" + big[6:], big[:9] + "T" + big[10:], big[:12] + "C" + big[13:])], dtype=np.uint64))
    add_list("B16", make_records(bw, [0xC0000000, 0xC0000001, 0x90000000, 0xFFFFFFFF][:len(bw)]), 16)
    # k = 32 with keys 0 and 2^64 - 1
    h = [0, 0xFFFFFFFFFFFFFFFF] + [M.canonical(word(seq(rng, 32)), 32) for _ in range(40)]
    add_list("K32", make_records(np.unique(np.array(h, dtype=np.uint64)), rng.integers(1, 9, size=42)), 32)
    # k = 25: every fifth canonical 25-mer of a random genome; reads are pieces of it with two substitutions
    genome = seq(rng, 3000)
    g25 = [word(genome[i:i + 25]) for i in range(0, len(genome) - 25, 5)]
    add_list("G25", canon_list(g25, 25, rng.integers(1, 9, size=len(g25))), 25)
    reads = []
    for r in range(30):
        p = int(rng.integers(0, len(genome) - 80))
        reads.append(">read%d some text\n%s\n" % (r, mutate(rng, genome[p:p + 80], 2)))
    add_file("reads25.fa", "".join(reads))
    # median: a list where the bisection stops early, one where max == min + 1 (both outcomes), one with equal counts
    add_list("MEDE", make_records(np.arange(1, 41, dtype=np.uint64) * 977, [1] * 10 + [7] * 5 + [8] * 5 + [9] * 10 + [100] * 9 + [1000]), 12)
    add_list("MED1", make_records(np.arange(1, 12, dtype=np.uint64) * 31, [4] * 3 + [5] * 8), 8)
    add_list("MED1B", make_records(np.arange(1, 12, dtype=np.uint64) * 31, [4] * 8 + [5] * 3), 8)
    add_list("MEDQ", make_records(np.arange(1, 8, dtype=np.uint64) * 31, [6] * 7), 8)
    add_list("MEDW", make_records(np.arange(1, 10, dtype=np.uint64) * 31, [1, 2, 3, 0xFFFFFFFF, 0xFFFFFFFE, 5, 5, 7, 0x80000000]), 8)

    # query files
    add_file("q16.txt", "\n".join([q16, "TAGCTGAGCGGCGAAC", "ACGTACGTACGTACGT", base16[0], base16[1].lower(), mutate(rng, base16[2], 1), mutate(rng, base16[3], 2)]) + "\n")
    add_file("q16_long.txt", "\n".join(["GG" + q16 + "TT", base16[0] + "ACGTAC", "\n" + "TTTT" + base16[5]]) + "\n")
    add_file("q16_bad.txt", "\n".join([q16, base16[0], "ACGT", base16[1]]) + "\n")
    add_file("q16_wrong.txt", "\n".join([base16[0], q16 + "A", base16[1]]) + "\n")
    add_file("q16_odd.txt", "\n".join([q16, "ACGTNNGTACGTACGT", "acgtacgtacgtacga\r", "  " + base16[4]]) + "\n")
    fa16 = (">one\n" + base16[0] + base16[1][:8] + "\n" + base16[1][8:] + "N" + q16 + "\n>short\nACGTACG\n>lower case\n" + base16[2].lower() + "acgt\n"
            ">crlf\r\n" + base16[3][:10] + "\r\n" + base16[3][10:] + "ACGTAC\r\n>x-y\n" + d1[0] + "-" + d2[0] + "*" + "ACGTACGTACGTACGT\n")
    add_file("s16.fa", fa16)
    add_file("s16.fq", "@r1\n" + base16[0] + "ACGT\n+\n" + "I" * 20 + "\n@r2 x\n" + q16 + "N" + d1[1] + "\n+r2\n" + "#" * 33 + "\n")
    add_file("bad_start.fa", "ACGT\n>x\nACGT\n")
    add_file("bad_plus.fq", "@r1\n" + base16[0] + "\n" + "I" * 16 + "\n")
    add_file("empty.fa", "")
    add_file("s8.fa", ">a\nACGTTGCANNACGTACGTTTGACCA\n>b\nTTGACCAGGTAC\n")
    add_file("q4.txt", "ACGT\nAAAA\nTTTT\nCGCG\nGATC\nTGCA\n")
    add_file("q32.txt", "A" * 32 + "\n" + "T" * 32 + "\n" + "A" * 31 + "C\n" + "ACGT" * 8 + "\n")
    add_file("q12.txt", "\n".join(seq(rng, 12) for _ in range(200)) + "\n")

    cases = []

    def run(cid, argv, keep_stderr=False):
        p = subprocess.run([REF] + argv, cwd=work, capture_output=True, timeout=300)
        assert p.returncode >= 0, (cid, p.returncode)  # no crash transcripts
        c = dict(id=cid, argv=argv, exit=p.returncode)
        out = p.stdout.decode("latin-1")
        if len(p.stdout) <= FULL_STDOUT:
            c["stdout"] = out
        else:
            c.update(stdout_sha256=hashlib.sha256(p.stdout).hexdigest(), stdout_bytes=len(p.stdout), stdout_head=out[:300])
        if keep_stderr:
            c["stderr"] = p.stderr.decode("latin-1")
        assert cid not in [x["id"] for x in cases], cid
        cases.append(c)

    # statistics
    for name in ("A8", "R1", "W1", "H1", "MEDE", "MED1", "MED1B", "MEDQ", "MEDW", "G25"):
        run("stat_" + name, [name + ".list", "--stat"])
        run("median_" + name, [name + ".list", "--median"])
        run("gc_" + name, [name + ".list", "--gc"])
    run("stat_two", ["A8.list", "B8.list", "-stat"])
    run("median_two", ["A8.list", "MED1.list", "--median"])
    for name, mx in (("A8", 8), ("A8", 3), ("R1", 20), ("MEDW", 4), ("MEDE", 5000), ("G25", 0)):
        run("distro_%s_%d" % (name, mx), [name + ".list", "--distribution", str(mx)])
    # dump of one list
    for name in ("A8", "H1", "K4", "E8", "Z16"):
        run("dump_" + name, [name + ".list"])
    # -q
    for mm in (0, 1, 2):
        run("q16_mm%d" % mm, ["L16.list", "-q", q16, "-mm", str(mm)])
        run("q16_all_mm%d" % mm, ["L16.list", "-q", q16, "-mm", str(mm), "--all"])
        run("q16_miss_mm%d" % mm, ["L16.list", "-q", "TTTTTTTTTTTTTTTT", "-mm", str(mm)])
    run("q16_mm3", ["L16.list", "-q", q16, "-mm", "3"])
    run("q16_all_mm3", ["L16.list", "-q", q16, "-mm", "3", "-all"])
    run("q16_rev", ["L16.list", "-q", M.word_to_string(M.revcomp(word(q16), 16), 16), "-mm", "2", "--all"])
    for p in (0, 4, 10, 14):
        run("q16_mm2_p%d" % p, ["L16.list", "-q", q16, "-mm", "2", "-p", str(p), "--all"])
    run("q16_mm2_p15_err", ["L16.list", "-q", q16, "-mm", "2", "-p", "15"], True)
    run("q16_mm0_p16", ["L16.list", "-q", q16, "-p", "16"])
    p = subprocess.run([REF, "L16.list", "-q", q16, "-mm", "2"], cwd=work, capture_output=True)
    v2 = int(p.stdout.split()[1])
    for lo, hi in ((v2, v2), (v2 + 1, None), (None, v2 - 1), (v2 - 1, v2 + 1), (1, None)):
        argv = ["L16.list", "-q", q16, "-mm", "2"] + (["-min", str(lo)] if lo is not None else []) + (["-max", str(hi)] if hi is not None else [])
        run("q16_mm2_min%s_max%s" % (lo, hi), argv)
    run("q16_miss_min1", ["L16.list", "-q", "TTTTTTTTTTTTTTTT", "-min", "1"])
    run("q16_all_min_ignored", ["L16.list", "-q", q16, "-mm", "2", "--all", "-min", "1000", "-max", "1"])
    # the palindrome, zero counts, wrapping sums
    for extra in ([], ["--all"], ["-min", "3"], ["-max", "1"]):
        run("pal_mm1" + "_".join([""] + extra).replace("-", ""), ["P16.list", "-q", "ACGTACGTACGTACGT", "-mm", "1"] + extra)
    run("pal_mm0", ["P16.list", "-q", "ACGTACGTACGTACGT"])
    for mm in (0, 1):
        for extra in ([], ["--all"], ["-min", "1"]):
            run("zero_mm%d" % mm + "_".join([""] + extra).replace("-", ""), ["Z16.list", "-q", "AAAACCCCGGGGTTTA", "-mm", str(mm)] + extra)
    for mm in (0, 1, 2):
        run("wrap_mm%d" % mm, ["B16.list", "-q", big, "-mm", str(mm)])
        run("wrap_all_mm%d" % mm, ["B16.list", "-q", big, "-mm", str(mm), "--all"])
    # k = 4, 8, 12, 25, 32
    for mm in (0, 1, 2, 3):
        run("f4_mm%d" % mm, ["K4.list", "-f", "q4.txt", "-mm", str(mm)])
    run("f4_mm4_all", ["K4.list", "-f", "q4.txt", "-mm", "4", "--all"])
    run("f4_mm2_p2_all", ["K4.list", "-f", "q4.txt", "-mm", "2", "-p", "2", "--all"])
    run("f4_mm2_p3_err", ["K4.list", "-f", "q4.txt", "-mm", "2", "-p", "3"], True)
    for mm in (0, 1, 2):
        run("f32_mm%d" % mm, ["K32.list", "-f", "q32.txt", "-mm", str(mm)])
        run("f32_all_mm%d" % mm, ["K32.list", "-f", "q32.txt", "-mm", str(mm), "--all"])
    run("f32_mm2_p30", ["K32.list", "-f", "q32.txt", "-mm", "2", "-p", "30", "--all"])
    run("f12_mm3", ["R1.list", "-f", "q12.txt", "-mm", "3"])
    run("f12_mm3_p5", ["R1.list", "-f", "q12.txt", "-mm", "3", "-p", "5", "-min", "1"])
    run("f12_mm2_all", ["R1.list", "-f", "q12.txt", "-mm", "2", "--all", "-min", "1"])
    run("s8_mm1", ["A8.list", "-s", "s8.fa", "-mm", "1"])
    run("s8_mm2_all", ["A8.list", "-s", "s8.fa", "-mm", "2", "--all"])
    for mm in (0, 1, 2):
        run("s25_mm%d" % mm, ["G25.list", "-s", "reads25.fa", "-mm", str(mm), "-min", "1"])
    run("s25_mm2_p10_all", ["G25.list", "-s", "reads25.fa", "-mm", "2", "-p", "10", "--all", "-min", "1"])
    run("s25_mm0_every", ["G25.list", "-s", "reads25.fa"])
    # -f: lengths, --3p / --5p, odd characters
    for mm in (0, 1, 2):
        run("f16_mm%d" % mm, ["L16.list", "-f", "q16.txt", "-mm", str(mm)])
    run("f16_all_mm2", ["L16.list", "-f", "q16.txt", "-mm", "2", "--all"])
    run("f16_long_3p", ["L16.list", "-f", "q16_long.txt", "--3p"])
    run("f16_long_5p", ["L16.list", "-f", "q16_long.txt", "--5p", "-mm", "1"])
    run("f16_long_err", ["L16.list", "-f", "q16_long.txt"], True)
    run("f16_short_err", ["L16.list", "-f", "q16_bad.txt", "-mm", "1"], True)
    run("f16_wrong_err", ["L16.list", "-f", "q16_wrong.txt"], True)
    run("f16_odd_3p", ["L16.list", "-f", "q16_odd.txt", "--3p", "-mm", "1"])
    run("f16_missing", ["L16.list", "-f", "nothere.txt"], True)
    run("q16_3p", ["L16.list", "-q", "GG" + q16, "--3p", "-mm", "1"])
    run("q16_5p", ["L16.list", "-q", q16 + "GG", "--5p", "-mm", "1"])
    run("q16_long_err", ["L16.list", "-q", q16 + "GG"], True)
    run("q16_short_err", ["L16.list", "-q", "ACGT"], True)
    run("q16_invalid_char", ["L16.list", "-q", "ACGTNNGTACGTACGT", "-mm", "1"])
    # -s
    for mm in (0, 1, 2):
        run("s16_fa_mm%d" % mm, ["L16.list", "-s", "s16.fa", "-mm", str(mm)])
        run("s16_fq_mm%d" % mm, ["L16.list", "-s", "s16.fq", "-mm", str(mm)])
    run("s16_fa_all_mm2", ["L16.list", "-s", "s16.fa", "-mm", "2", "--all"])
    run("s16_fa_mm1_p8_min1", ["L16.list", "-s", "s16.fa", "-mm", "1", "-p", "8", "-min", "1"])
    run("s16_bad_start", ["L16.list", "-s", "bad_start.fa"])
    run("s16_bad_plus", ["L16.list", "-s", "bad_plus.fq"])
    run("s16_empty", ["L16.list", "-s", "empty.fa"])
    # (a sequence file that is not there: the reference reads from the unopened source and fails an assertion,
    # exit 255; the product prints search_fasta's message and exits 1 -- tests/test_gquery_cli.py, not a transcript)
    # -l
    run("l8_mm0", ["A8.list", "-l", "B8.list"])
    for mm in (1, 2):
        run("l8_mm%d" % mm, ["A8.list", "-l", "B8.list", "-mm", str(mm)])
        run("l12_mm%d_min1" % mm, ["R1.list", "-l", "R2.list", "-mm", str(mm), "-min", "1", "-max", "40"])
    run("l8_mm1_all", ["A8.list", "-l", "B8.list", "-mm", "1", "--all"])
    run("l8_mm0_p2", ["A8.list", "-l", "B8.list", "-p", "2"])
    # early errors and the rest of the grammar
    run("err_no_list", ["-q", "ACGT"], True)
    run("err_unknown", ["A8.list", "--nonsense"], True)
    run("err_multi_query", ["A8.list", "B8.list", "-q", "ACGTACGT"], True)
    run("err_multi_mm", ["A8.list", "B8.list", "-l", "M0.list", "-mm", "1"], True)
    run("err_multi_p", ["A8.list", "B8.list", "-l", "M0.list", "-p", "1"], True)
    run("err_wordlength", ["A8.list", "K9.list"], True)
    run("err_wordlength_query_list", ["A8.list", "-l", "K9.list"])
    run("err_missing_list", ["nothere.list", "--stat"], True)
    run("err_mm_17", ["A8.list", "-q", "ACGTACGT", "-mm", "17"], True)
    run("err_p_33", ["A8.list", "-q", "ACGTACGT", "-p", "33"], True)
    run("err_mm_text", ["A8.list", "-q", "ACGTACGT", "-mm", "x"], True)
    run("err_mm_last", ["A8.list", "-mm"], True)
    run("err_min_text", ["A8.list", "-q", "ACGTACGT", "-min", "1x"], True)
    run("err_distribution_last", ["A8.list", "--distribution"], True)
    run("warn_no_query", ["A8.list", "-q", "--stat"], True)
    run("version", ["-v"], True)
    run("help", ["-h"], True)
    run("header_multi", ["M0.list", "M1.list", "--header"])
    run("bloom_scouts_ignored", ["L16.list", "-q", q16, "-mm", "1", "--bloom", "--disable_scouts"])

    def pack(rec):
        return base64.b64encode(zlib.compress(np.ascontiguousarray(rec, dtype=RECORD_DTYPE).tobytes(), 9)).decode()

    out = dict(inputs=inputs, lists={n: [pack(r), k] for n, (r, k) in lists.items()}, files=files, cases=cases)
    with open(os.path.join(HERE, "gquery_cases.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print("%d cases, %d bytes, %.1f s" % (len(cases), os.path.getsize(os.path.join(HERE, "gquery_cases.json")), time.time() - t0))


if __name__ == "__main__":
    main()
