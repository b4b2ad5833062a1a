#!/usr/bin/env python3
"""Expected output of `glistquery LIST -s FILE --mask [--soft_mask]`, from the reference's glistquery alone.

The option is not the reference's, its result is.  The reference's `glistquery LIST -s FILE` prints, with default options,
one line CANONICAL_WORD <tab> VALUE per word of the file in text order, absent words with 0.  For every case each sequence
of FILE is written into a file of its own and the reference runs on it twice:

    with defaults                                  line i is word i
    with -min max (A, 1) -max B and the -mm / -p   the set H of first columns is the hit words

Whether a word is a hit depends on its canonical form alone, so word i is a hit iff its string is in H.  Where word i's k
bases stand is found here by a scan of the sequence (runs broken at any byte >= ' ' that is no base, bytes < ' ' skipped);
it is ASSERTED that the reference's string for line i is the canonical form of exactly those bases, and that the second
run's lines are the first run's filtered by H, in order.  The expected stdout is the file with the covered bases replaced.
Needs oracle/_ref/glistquery (make -C oracle ref).  Writes tests/golden/gqmask_cases.json (data only):

    lists    {name: [zlib + base64 of the packed 12-byte records, word length]}
    files    {name: text} (latin-1)
    cases    [{id, kind, argv, exit, stdout, counts, stderr}]; kind "computed": counts = [words, hits, covered bases] of the
             file; "malformed": a FastQ file whose last record has no '+' line: stdout is the masked form of the bytes in
             front of the offending byte, from the records as well-formed files of their own, exit and stderr the
             reference's on the whole file; "argv": refused by the rules of the option, exit 1, nothing on stdout."""
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
BASES = "ACGTUacgtu"


def seq(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, size=n))


def canon_string(s):
    k = len(s)
    return M.word_to_string(M.canonical(M.string_to_word(s.upper().replace("U", "T"), k), k), k)


def record_text(kind, rec, eol="\n", defect=False):
    """one record as it stands in its file; FastQ quality lines are made of the letters A C G T"""
    name, lines = rec
    if kind == "fa":
        return ">" + name + eol + "".join(l + eol for l in lines)
    assert len(lines) == 1
    qual = ("TGCA" * len(lines[0]))[:len(lines[0])]
    return "@" + name + eol + lines[0] + eol + ("" if defect else "+" + eol) + qual + eol


def word_bases(kind, text, k):
    """the offsets of the k bases of every word of a one-record file, in text order"""
    first_nl = text.index("\n")
    end = len(text) if kind == "fa" else text.index("\n", first_nl + 1)
    run, out = [], []
    for i in range(first_nl + 1, end):
        ch = text[i]
        if ch in BASES:
            run.append(i)
            if len(run) >= k:
                out.append(run[-k:])
        elif ch >= " ":
            run = []
    return out


def main():
    if not os.path.exists(REF):
        sys.exit("build the reference first: make -C oracle ref")
    t0 = time.time()
    rng = np.random.default_rng(2025)
    work = tempfile.mkdtemp(prefix="gt4gqmask_")
    lists, files, records, cases, memo = {}, {}, {}, [], {}

    def add_list(name, words, counts, k):
        keys = np.array([M.canonical(M.string_to_word(w.upper().replace("U", "T"), k), k) if isinstance(w, str) else w for w in words], dtype=np.uint64)
        keys, idx = np.unique(keys, return_index=True)
        rec = make_records(keys, np.asarray(counts, dtype=np.uint32)[idx])
        lists[name] = (rec, k)
        write_list(os.path.join(work, name + ".list"), rec, k)

    def add_file(name, kind, recs, eol="\n", defect=False):
        parts = [record_text(kind, r, eol, defect and i == len(recs) - 1) for i, r in enumerate(recs)]
        files[name] = "".join(parts)
        records[name] = (kind, recs, eol, parts)
        with open(os.path.join(work, name), "wb") as f:
            f.write(files[name].encode("latin-1"))

    def ref_lines(lst, text, extra):
        key = (lst, text, tuple(extra))
        if key not in memo:
            with open(os.path.join(work, "one_sequence"), "wb") as f:
                f.write(text.encode("latin-1"))
            p = subprocess.run([REF, lst + ".list", "-s", "one_sequence"] + list(extra), cwd=work, capture_output=True, timeout=300)
            assert p.returncode == 0, (key, p.returncode, p.stderr)
            memo[key] = [l.split("\t") for l in p.stdout.decode("latin-1").splitlines()]
        return memo[key]

    def masked(lst, fname, mm, pm, lo, hi, soft, upto=None):
        kind, recs, eol, parts = records[fname]
        k = lists[lst][1]
        out = list(files[fname])
        n_words = n_hits = 0
        covered = set()
        off = 0
        for rec, part in zip(recs, parts):
            text = record_text(kind, rec, eol)  # (well formed, also where `part` is not)
            one = ref_lines(lst, text, [])
            extra = ["-min", str(max(lo, 1)), "-max", str(hi)] + (["-mm", str(mm)] if mm else []) + (["-p", str(pm)] if pm else [])
            hits = ref_lines(lst, text, extra)
            H = {h[0] for h in hits}
            where = word_bases(kind, text, k)
            assert len(where) == len(one), (fname, rec[0], len(where), len(one))
            for line, pos in zip(one, where):
                assert line[0] == canon_string("".join(text[p] for p in pos)), (fname, rec[0], line, pos)
            assert [h[0] for h in hits] == [l[0] for l in one if l[0] in H], (fname, rec[0])
            for line, pos in zip(one, where):
                n_words += 1
                if line[0] in H:
                    n_hits += 1
                    covered.update(off + p for p in pos)
            off += len(part)
        for p in covered:
            assert out[p] in BASES and files[fname][p] == out[p]
            out[p] = chr(ord(out[p]) | 0x20) if soft else "N"
        return "".join(out)[:upto], [n_words, n_hits, len(covered)]

    def computed(cid, lst, fname, mm=0, pm=0, lo=None, hi=None, soft=False, kind="computed", exit_code=0, upto=None, stderr=""):
        out, counts = masked(lst, fname, mm, pm, 0 if lo is None else lo, 0xFFFFFFFF if hi is None else hi, soft, upto)
        argv = [lst + ".list", "-s", fname, "--mask"] + (["--soft_mask"] if soft else [])
        argv += (["-mm", str(mm)] if mm else []) + (["-p", str(pm)] if pm else [])
        argv += (["-min", str(lo)] if lo is not None else []) + (["-max", str(hi)] if hi is not None else [])
        assert cid not in [c["id"] for c in cases], cid
        cases.append(dict(id=cid, kind=kind, argv=argv, exit=exit_code, stdout=out, counts=counts, stderr=stderr))
        return out, counts

    def refused(cid, argv):
        cases.append(dict(id=cid, kind="argv", argv=argv, exit=1, stdout="", counts=[], stderr=""))

    def n_runs(s, k):
        """s with N-broken runs of k - 1, k and k + 1 bases in front of it"""
        return s[:k - 1] + "N" + s[k:2 * k] + "N" + s[2 * k + 1:3 * k + 2] + "N" + s[3 * k + 3:]

    # ---- the files.  Sequences shorter than any k first, in the middle and last; lines that break a sequence and an empty
    # line inside one; lower case and U; N-broken runs of k - 1, k and k + 1 for k = 4 and 9; names and quality lines made of
    # the letters A C G T
    body = [seq(rng, n) for n in (70, 60, 64, 61, 58, 45, 52)]
    small = [("ACG short first", ["AC"]), ("ACGTACGTACGTACGT three lines", [body[0][:20], body[0][20:41], body[0][41:]]), ("", [body[1]]),
             ("n-runs-9\tx", [n_runs(body[2], 9)]), ("GATTACA", ["A"]), ("TTTT ", ["ACG"]), ("n-runs-4", [n_runs(body[5][:24], 4)]),
             ("lower case and U", [body[3][:30].lower().replace("t", "u"), body[3][30:].replace("T", "U")]),
             ("empty line inside", [body[4][:24], "", body[4][24:]]), ("nN", ["NNNNACGNNNN"]), ("tail", [body[6]]), ("short last", ["TT"])]
    add_file("small.fa", "fa", small)
    small_q = [(n, ["".join(l)]) for n, l in small]
    add_file("small.fq", "fq", small_q)
    add_file("crlf.fa", "fa", small[:4], eol="\r\n")
    add_file("crlf.fq", "fq", small_q[:4], eol="\r\n")
    genome = seq(rng, 400)
    g = [("g0", [genome[0:20]]), ("ACGT one", [genome[10:60], genome[60:160]]), ("", [genome[150:190] + "N" + genome[191:250]]), ("g3", [genome[260:284]]),
         ("g4", ["ACGT"]), ("exact 25", [genome[300:325]]), ("n-runs-25", [n_runs(genome[200:330], 25)]), ("end", [genome[0:24]])]
    add_file("g25.fa", "fa", g)
    add_file("g25.fq", "fq", [(n, ["".join(l)]) for n, l in g])

    # ---- the lists
    all4 = sorted({M.canonical(w, 4) for w in range(256)})
    add_list("K4ALL", all4, rng.integers(1, 50, size=len(all4)), 4)
    third4 = all4[::3]
    add_list("K4", third4, rng.integers(1, 50, size=len(third4)), 4)

    def text_words(fname, k):
        """the word strings of a file's records in text order, record by record"""
        kind, recs, eol, _ = records[fname]
        out = []
        for rec in recs:
            text = record_text(kind, rec, eol)
            out.append([canon_string("".join(text[p] for p in pos)) for pos in word_bases(kind, text, k)])
        return out

    def spaced(words, k):
        """words of one sequence whose covers overlap, touch, and leave gaps of 1 and of k - 1 bases"""
        at, picks = 0, []
        for step in (0, 3, k, k + 1, 2 * k - 1):
            at += step
            picks.append(words[at])
        return picks

    w9 = text_words("small.fa", 9)
    flat9 = [w for ws in w9 for w in ws]
    long9 = w9[2]  # the 60 bases of one line
    assert len(set(long9)) == len(long9) and len(long9) > 5 * 9
    pat9 = spaced(long9, 9)
    assert not (set(pat9) & (set(flat9) - set(long9))) and all(flat9.count(w) == 1 for w in pat9)
    add_list("PAT9", pat9, [7] * len(pat9), 9)
    every3 = flat9[::3]
    other = [int(x) for x in rng.integers(0, 1 << 18, size=3000)]
    other = sorted({M.canonical(x, 9) for x in other} - {M.string_to_word(w, 9) for w in flat9})
    add_list("K9", every3 + other, rng.integers(1, 30, size=len(every3) + len(other)), 9)
    add_list("NONE9", other[:500], rng.integers(1, 30, size=500), 9)
    add_list("ALL9", sorted(set(flat9)), rng.integers(1, 30, size=len(set(flat9))), 9)
    add_list("Z9", every3, [0 if i % 2 == 0 else 3 for i in range(len(every3))], 9)
    vw = w9[1][:40:10]  # four words of one sequence, ten bases apart: values at A - 1, A, B and B + 1 for -min 5 -max 9
    assert len(set(vw)) == 4 and all(flat9.count(w) == 1 for w in vw)
    add_list("V9", vw, [4, 5, 9, 10], 9)
    w25 = text_words("g25.fa", 25)
    flat25 = [w for ws in w25 for w in ws]
    pat25 = spaced(w25[1], 25)
    add_list("PAT25", pat25, [2] * len(pat25), 25)
    add_list("G25", flat25[::3], rng.integers(1, 9, size=len(flat25[::3])), 25)

    # ---- the cases
    for soft in (False, True):
        s = "_soft" if soft else ""
        computed("k4_all_fa" + s, "K4ALL", "small.fa", soft=soft)
        computed("k4_fq" + s, "K4", "small.fq", soft=soft)
        computed("k9_fa" + s, "K9", "small.fa", soft=soft)
        computed("k9_fq" + s, "K9", "small.fq", soft=soft)
        computed("k25_fa" + s, "G25", "g25.fa", soft=soft)
        computed("k9_crlf_fa" + s, "K9", "crlf.fa", soft=soft)
        computed("k9_crlf_fq" + s, "ALL9", "crlf.fq", soft=soft)
    computed("k4_fa", "K4", "small.fa")
    computed("k4_all_fq", "K4ALL", "small.fq")
    computed("k25_fq", "G25", "g25.fq")
    out, counts = computed("k9_all_fa", "ALL9", "small.fa")
    assert counts[0] == counts[1] > 0
    out, counts = computed("k9_none_fa", "NONE9", "small.fa")
    assert counts[1:] == [0, 0] and out == files["small.fa"]
    computed("k9_none_fq_soft", "NONE9", "small.fq", soft=True)
    for lst, fname, k, name in (("PAT9", "small.fa", 9, ""), ("PAT25", "g25.fa", 25, "ACGT one")):
        out, counts = computed("pattern_k%d" % k, lst, fname)
        line = out[out.index(">" + name + "\n") + len(name) + 2:]
        line = line[:line.index(">")].replace("\n", "")  # the sequence the words were picked from
        runs = [len(r) for r in line.replace("N", " ").split()]  # the bases left between the covers
        assert counts[1] == 5 and 1 in runs and k - 1 in runs and "N" * (2 * k) in line and "N" * (k + 3) in line, (line, runs)
        computed("pattern_k%d_soft" % k, lst, fname, soft=True)
    computed("zero_fa", "Z9", "small.fa")
    computed("zero_fa_min0", "Z9", "small.fa", 0, 0, 0)
    computed("zero_fa_mm1", "Z9", "small.fa", 1)
    for lo, hi, n in ((5, 9, 2), (4, 10, 4), (6, 8, 0), (10, 10, 1), (4, 4, 1), (None, 4, 1), (10, None, 1)):
        out, counts = computed("bounds_min%s_max%s" % (lo, hi), "V9", "small.fa", 0, 0, lo, hi)
        assert counts[1] == n, (lo, hi, counts)
    computed("k4_fa_mm1", "K4", "small.fa", 1)
    computed("k4_fq_mm2_p2", "K4", "small.fq", 2, 2)
    computed("k9_fa_mm1", "K9", "small.fa", 1)
    computed("k9_fa_mm1_soft", "K9", "small.fa", 1, soft=True)
    computed("k9_fq_mm2_p3", "K9", "small.fq", 2, 3)
    computed("k9_fa_mm2_p3_min3_max40", "K9", "small.fa", 2, 3, 3, 40)
    computed("k25_fa_mm1", "G25", "g25.fa", 1)
    computed("k25_fq_mm2_p3", "G25", "g25.fq", 2, 3)

    # one malformed FastQ: the last record has no '+' line; the reference has read its whole sequence line by then
    bad = small_q[1:4]
    add_file("bad.fq", "fq", bad, defect=True)
    p = subprocess.run([REF, "K9.list", "-s", "bad.fq"], cwd=work, capture_output=True, timeout=300)
    assert p.returncode > 0 and b"tag '+' missing" in p.stderr, (p.returncode, p.stderr)
    parts = records["bad.fq"][3]
    upto = len("".join(parts[:-1])) + parts[-1].index("\n", parts[-1].index("\n") + 1) + 1  # behind the last sequence line
    err = [l for l in p.stderr.decode("latin-1").splitlines() if "missing" in l][0]
    for soft in (False, True):
        computed("malformed_fq" + ("_soft" if soft else ""), "K9", "bad.fq", soft=soft, kind="malformed", exit_code=p.returncode, upto=upto, stderr=err)

    files["z.fa.gz"] = "\x1f\x8b\x08\x00rest"
    files["q.txt"] = "ACGTACGTA\n"
    mask = ["--mask"]
    refused("err_no_s", ["K9.list"] + mask)
    refused("err_q", ["K9.list", "-s", "small.fa", "-q", "ACGTACGTA"] + mask)
    refused("err_f", ["K9.list", "-s", "small.fa", "-f", "q.txt"] + mask)
    refused("err_l", ["K9.list", "-s", "small.fa", "-l", "Z9.list"] + mask)
    refused("err_all", ["K9.list", "-s", "small.fa", "--all"] + mask)
    refused("err_locations", ["K9.list", "-s", "small.fa", "--locations"] + mask)
    refused("err_files", ["K9.list", "-s", "small.fa", "--files"] + mask)
    refused("err_sequences", ["K9.list", "-s", "small.fa", "--sequences"] + mask)
    refused("err_per_sequence", ["K9.list", "-s", "small.fa", "--per_sequence"] + mask)
    refused("err_min_hits", ["K9.list", "-s", "small.fa", "--min_hits", "2"] + mask)
    for opt in (["--stat"], ["--median"], ["--gc"], ["--distribution", "3"]):
        refused("err_" + opt[0].strip("-"), ["K9.list", "-s", "small.fa"] + mask + opt)
    refused("err_soft_alone", ["K9.list", "-s", "small.fa", "--soft_mask"])
    refused("err_two_lists", ["K9.list", "Z9.list", "-s", "small.fa"] + mask)
    refused("err_gzip", ["K9.list", "-s", "z.fa.gz"] + mask)

    def pack(rec):
        return base64.b64encode(zlib.compress(np.ascontiguousarray(rec, dtype=RECORD_DTYPE).tobytes(), 9)).decode()

    out = dict(lists={n: [pack(r), k] for n, (r, k) in lists.items()}, files=files, cases=cases)
    path = os.path.join(HERE, "gqmask_cases.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print("%d cases, %d bytes, %.1f s" % (len(cases), os.path.getsize(path), time.time() - t0))
    assert os.path.getsize(path) < 200_000


if __name__ == "__main__":
    main()
