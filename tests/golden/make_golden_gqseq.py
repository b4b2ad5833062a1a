#!/usr/bin/env python3
"""Expected output of `glistquery LIST -s FILE --per_sequence`, from the reference's glistquery alone.

The option is not the reference's, its result is: for every case each sequence of FILE is written into a file of its own
and the reference's `glistquery LIST -s` runs on it twice:

    with defaults                                  one line per word: the line count is WORDS
    with -min max (A, 1) -max B and the -mm / -p   one line per hit: the line count is HITS, the second column adds up to SUM

NAME is the name line up to its first byte <= ' '.  The expected stdout is NAME, WORDS, HITS, SUM per sequence with
HITS >= --min_hits, in file order.  Needs oracle/_ref/glistquery (make -C oracle ref).  Writes tests/golden/gqseq_cases.json:

    lists    {name: [zlib + base64 of the packed 12-byte records, word length]} (data only)
    files    {name: text} (latin-1)
    cases    [{id, kind, argv, exit, stdout, rows}]; kind "computed": rows = [NAME, WORDS, HITS, SUM] of every sequence, from
             the reference; "malformed": the same for the records in front of the defect (each as a well-formed file of its
             own; the reference reads the whole sequence line before it misses the '+'), exit = the reference's on the
             whole file; "argv": refused by the rules of the option, exit 1 and nothing on stdout."""
import base64
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


def word(s):
    return M.string_to_word(s, len(s))


def seq(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, size=n))


def words_of(text, k):
    """canonical words of a plain sequence string, runs broken at anything but a base"""
    out, run = [], ""
    for ch in text + "#":
        if ch in "ACGTacgt":
            run += ch.upper()
            if len(run) >= k:
                out.append(M.canonical(word(run[-k:]), k))
        elif ch >= " ":
            run = ""
    return out


def whole(kind, recs, defect=False):
    """the file of these records; defect: the last FastQ record has no '+' line"""
    if kind == "fa":
        return "".join(">%s\n%s" % (name, "".join(l + "\n" for l in lines)) for name, lines in recs)
    out = ""
    for i, (name, lines) in enumerate(recs):
        assert len(lines) == 1
        plus = "" if defect and i == len(recs) - 1 else "+\n"
        out += "@%s\n%s\n%s%s\n" % (name, lines[0], plus, "I" * len(lines[0]))
    return out


def main():
    if not os.path.exists(REF):
        sys.exit("build the reference first: make -C oracle ref")
    t0 = time.time()
    rng = np.random.default_rng(2024)
    work = tempfile.mkdtemp(prefix="gt4gqseq_")
    lists, files, records, cases, memo = {}, {}, {}, [], {}

    def add_list(name, keys, counts, k):
        keys = np.asarray(keys, dtype=np.uint64)
        order = np.argsort(keys)
        rec = make_records(keys[order], np.asarray(counts, dtype=np.uint32)[order])
        assert len(np.unique(keys)) == len(keys)
        lists[name] = (rec, k)
        write_list(os.path.join(work, name + ".list"), rec, k)

    def add_file(name, kind, recs, defect=False):
        files[name] = whole(kind, recs, defect)
        records[name] = (kind, recs)
        with open(os.path.join(work, name), "wb") as f:
            f.write(files[name].encode("latin-1"))

    def ref_lines(lst, kind, rec, extra):
        """the reference's lines for one record in a file of its own"""
        key = (lst, kind, rec[0], tuple(rec[1]), tuple(extra))
        if key not in memo:
            with open(os.path.join(work, "one_sequence"), "wb") as f:
                f.write(whole(kind, [rec]).encode("latin-1"))
            p = subprocess.run([REF, lst + ".list", "-s", "one_sequence"] + list(extra), cwd=work, capture_output=True, timeout=300)
            assert p.returncode == 0, (key, p.returncode, p.stderr)
            memo[key] = [l.split("\t") for l in p.stdout.decode("latin-1").splitlines()]
        return memo[key]

    def rows_of(lst, fname, mm, pm, lo, hi):
        kind, recs = records[fname]
        rows = []
        for rec in recs:
            n_words = len(ref_lines(lst, kind, rec, []))
            extra = ["-min", str(max(lo, 1)), "-max", str(hi)] + (["-mm", str(mm)] if mm else []) + (["-p", str(pm)] if pm else [])
            hits = ref_lines(lst, kind, rec, extra)
            name = rec[0]
            for i, ch in enumerate(name):
                if ch <= " ":
                    name = name[:i]
                    break
            rows.append([name, n_words, len(hits), sum(int(h[1]) for h in hits)])
        return rows

    def computed(cid, lst, fname, mm=0, pm=0, lo=None, hi=None, min_hits=None, kind="computed", exit_code=0):
        rows = rows_of(lst, fname, mm, pm, 0 if lo is None else lo, 0xFFFFFFFF if hi is None else hi)
        argv = [lst + ".list", "-s", fname, "--per_sequence"]
        argv += (["-mm", str(mm)] if mm else []) + (["-p", str(pm)] if pm else [])
        argv += (["-min", str(lo)] if lo is not None else []) + (["-max", str(hi)] if hi is not None else [])
        argv += ["--min_hits", str(min_hits)] if min_hits is not None else []
        out = "".join("%s\t%d\t%d\t%d\n" % tuple(r) for r in rows if r[2] >= (min_hits or 0))
        assert cid not in [c["id"] for c in cases], cid
        cases.append(dict(id=cid, kind=kind, argv=argv, exit=exit_code, stdout=out, rows=rows))
        return rows

    def refused(cid, argv):
        cases.append(dict(id=cid, kind="argv", argv=argv, exit=1, stdout="", rows=[]))

    # ---- the sequences: short ones (fewer bases than any k here) first, last and three in a row in the middle; lines that
    # break a sequence; runs broken by N; an empty name; names with spaces and a tab
    body = [seq(rng, n) for n in (57, 40, 33, 61, 48, 25, 52)]
    small = [("s0 short first", ["AC"]), ("one two three", [body[0][:20], body[0][20:41], body[0][41:]]), ("", [body[1]]),
             ("n-runs\tx", [body[2][:9] + "N" + body[2][9:20] + "NN" + body[2][20:]]), ("s1", ["A"]), ("s2 ", []), ("s3", ["ACG"]),
             ("lower case", [body[3][:30].lower(), body[3][30:]]), ("dup", [body[0][:30]]), ("x|y;z", [body[4][:24], "", body[4][24:]]),
             ("nN", ["NNNNACGNNNN"]), ("tail", [body[5], body[6]]), ("short last", ["TTT"])]
    add_file("small.fa", "fa", small)
    small_q = [(n, ["".join(l)]) for n, l in small]
    add_file("small.fq", "fq", small_q)
    genome = seq(rng, 1500)
    g = [("g0", [genome[0:20]]), ("read one", [genome[10:60], genome[60:100]]), ("", [genome[200:240] + "N" + genome[241:300]]),
         ("g3", [genome[400:424]]), ("g4", ["ACGT"]), ("g5", [""]), ("mut 1", [genome[500:530] + "T" + genome[531:580]]),
         ("elsewhere", [seq(rng, 70)]), ("exact 25", [genome[700:725]]), ("g9", [genome[900:960], genome[960:990]]), ("end", [genome[0:24]])]
    add_file("g25.fa", "fa", g)
    add_file("g25.fq", "fq", [(n, ["".join(l)]) for n, l in g])

    # ---- the lists
    all4 = sorted({M.canonical(w, 4) for w in range(256)})
    add_list("K4ALL", all4, rng.integers(1, 50, size=len(all4)), 4)
    k4 = [w for i, w in enumerate(all4) if i % 9]  # nearly every word hits
    add_list("K4", k4, rng.integers(1, 50, size=len(k4)), 4)
    w9 = sorted(set(words_of("".join("".join(l) + "#" for _, l in small), 9)))
    keep = [w for i, w in enumerate(w9) if i % 3 != 2]
    other = sorted({M.canonical(int(x), 9) for x in rng.integers(0, 1 << 18, size=4000)} - set(w9))
    add_list("K9", keep + other, rng.integers(1, 30, size=len(keep) + len(other)), 9)
    # stored counts of 0 among the words of the file
    add_list("Z9", keep, [0 if i % 4 == 0 else 3 for i in range(len(keep))], 9)
    # values exactly at A - 1, A, B and B + 1 for -min 5 -max 9, in one sequence; the rest far off
    vw = words_of(body[0][:20], 9)
    assert len(set(vw)) == len(vw) >= 8
    add_list("V9", vw[:8], [4, 5, 9, 10, 1, 7, 200, 6], 9)
    # 0xFFFFFFFF twice in one sequence
    bw = words_of(body[1], 9)
    assert len(set(bw[:6])) == 6
    add_list("BIG9", bw[:6], [0xFFFFFFFF, 1, 0xFFFFFFFF, 2, 0xFFFFFFFE, 3], 9)
    g25 = sorted(set(words_of(genome, 25)))
    g25 = [w for i, w in enumerate(g25) if i % 5 != 4]
    add_list("G25", g25, rng.integers(1, 9, size=len(g25)), 25)
    # every sequence has hits: words of K4ALL only, every sequence at least four bases
    add_file("allhit.fa", "fa", [("a", [body[0][:12]]), ("b c", [body[1][:7], body[1][7:19]]), ("", ["ACGT"])])

    # ---- the cases
    for k, lst in ((4, "K4"), (9, "K9")):
        computed("k%d_fa" % k, lst, "small.fa")
        computed("k%d_fq" % k, lst, "small.fq")
    computed("k4_fa_mm1", "K4", "small.fa", 1)
    computed("k4_fa_mm2_p1", "K4", "small.fa", 2, 1)  # variants that share a canonical form count twice
    computed("k4_fq_mm2_p2", "K4", "small.fq", 2, 2)
    computed("k4_fa_mm1_p3_max60", "K4", "small.fa", 1, 3, None, 60)
    computed("k9_fa_mm1", "K9", "small.fa", 1)
    computed("k9_fa_mm2_p3", "K9", "small.fa", 2, 3)
    computed("k9_fq_mm1_p2", "K9", "small.fq", 1, 2)
    computed("k9_fa_p4_only", "K9", "small.fa", 0, 4)
    computed("k25_fa", "G25", "g25.fa")
    computed("k25_fq", "G25", "g25.fq")
    computed("k25_fa_mm1", "G25", "g25.fa", 1)
    computed("k25_fa_mm2_p10", "G25", "g25.fa", 2, 10)
    computed("zero_fa", "Z9", "small.fa")
    computed("zero_fa_min0", "Z9", "small.fa", 0, 0, 0)
    computed("zero_fa_mm1", "Z9", "small.fa", 1)
    for lo, hi in ((5, 9), (4, 10), (6, 8), (0, 9), (5, None), (None, 4), (10, 10), (11, 199)):
        computed("bounds_min%s_max%s" % (lo, hi), "V9", "small.fa", 0, 0, lo, hi)
    computed("bounds_mm1_min5_max9", "V9", "small.fa", 1, 0, 5, 9)
    rows = computed("big_fa", "BIG9", "small.fa")
    assert max(r[3] for r in rows) > 1 << 32
    computed("big_fq_max", "BIG9", "small.fq", 0, 0, 1, 0xFFFFFFFF)
    computed("big_fa_max_fffffffe", "BIG9", "small.fa", 0, 0, None, 0xFFFFFFFE)
    rows = computed("allhit_fa", "K4ALL", "allhit.fa")
    assert all(r[2] > 0 for r in rows)
    rows = [c for c in cases if c["id"] == "k9_fa"][0]["rows"]
    h = sorted({r[2] for r in rows})[-2]  # a sequence's HITS, with sequences above and below it
    assert h > 1 and any(r[2] == 0 for r in rows)
    for mh in (h, h - 1, h + 1, 0, 1, 10 ** 12):
        computed("min_hits_%d" % mh, "K9", "small.fa", min_hits=mh)
    computed("min_hits_1_k25_fq_mm1", "G25", "g25.fq", 1, min_hits=1)

    # one malformed FastQ: the third record has no '+' line; the reference has read its whole sequence line by then
    bad = small_q[1:4]
    add_file("bad.fq", "fq", bad, defect=True)
    p = subprocess.run([REF, "K9.list", "-s", "bad.fq"], cwd=work, capture_output=True, timeout=300)
    assert p.returncode > 0 and b"tag '+' missing" in p.stderr, (p.returncode, p.stderr)
    computed("malformed_fq", "K9", "bad.fq", kind="malformed", exit_code=p.returncode)

    files["z.fa.gz"] = "\x1f\x8b\x08\x00rest"
    files["q.txt"] = "ACGTACGTA\n"
    per = ["--per_sequence"]
    refused("err_no_s", ["K9.list"] + per)
    refused("err_q", ["K9.list", "-s", "small.fa", "-q", "ACGTACGTA"] + per)
    refused("err_f", ["K9.list", "-s", "small.fa", "-f", "q.txt"] + per)
    refused("err_l", ["K9.list", "-s", "small.fa", "-l", "Z9.list"] + per)
    refused("err_all", ["K9.list", "-s", "small.fa", "--all"] + per)
    refused("err_locations", ["K9.list", "-s", "small.fa", "--locations"] + per)
    refused("err_files", ["K9.list", "-s", "small.fa", "--files"] + per)
    refused("err_sequences", ["K9.list", "-s", "small.fa", "--sequences"] + per)
    for opt in (["--stat"], ["--median"], ["--gc"], ["--distribution", "3"]):
        refused("err_" + opt[0].strip("-"), ["K9.list", "-s", "small.fa"] + per + opt)
    refused("err_min_hits_alone", ["K9.list", "-s", "small.fa", "--min_hits", "2"])
    refused("err_min_hits_text", ["K9.list", "-s", "small.fa", "--min_hits", "x"] + per)
    refused("err_two_lists", ["K9.list", "Z9.list", "-s", "small.fa"] + per)
    refused("err_gzip", ["K9.list", "-s", "z.fa.gz"] + per)

    def pack(rec):
        return base64.b64encode(zlib.compress(np.ascontiguousarray(rec, dtype=RECORD_DTYPE).tobytes(), 9)).decode()

    assert any(c["kind"] == "computed" and c["rows"] and all(r[2] > 0 for r in c["rows"]) for c in cases)
    assert any(c["kind"] == "computed" and any(r[2] == 0 for r in c["rows"]) for c in cases)
    out = dict(lists={n: [pack(r), k] for n, (r, k) in lists.items()}, files=files, cases=cases)
    path = os.path.join(HERE, "gqseq_cases.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print("%d cases, %d bytes, %.1f s" % (len(cases), os.path.getsize(path), time.time() - t0))


if __name__ == "__main__":
    main()
