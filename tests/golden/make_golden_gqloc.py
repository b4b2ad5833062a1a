#!/usr/bin/env python3
"""Golden transcripts of the reference's glistquery on GT4I indexes: --files, --sequences, --locations without a query
(the whole index) and with -q / -f / -s / -l (reference src/glistquery.c:439-568, :702-717).

Needs oracle/_ref/glistquery and oracle/_ref/glistmaker (make -C oracle ref).  The indexes are the reference-built ones
of tests/golden/gindex_files.npz (their four masked bytes play no part in a query), written under their output names
beside the source texts of gindex_cases.json; long_k16 and big_k25, too large to be kept, are built here with the
reference's glistmaker.  Writes tests/golden/gqloc_cases.json (data only):

    files    {name: text}: query files and reads made here (latin-1)
    lists    {name: [[word, count], ...]}: the small query list, word length LIST_K
    built    ids of gindex_cases.json a replay has to build itself (glistmaker --index)
    cases    [{id, argv, exit, stdout | (stdout_sha256, stdout_bytes, stdout_head), stderr (where kept)}]

Every case with --locations in a query form is followed by the same argv without it (id + "_plain")."""
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gindex_util as G  # noqa: E402
import query_model as M  # noqa: E402
from genometester4_amd.listio import make_records, write_list  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "glistquery")
REF_MAKER = os.path.join(ROOT, "oracle", "_ref", "glistmaker")
OUT = os.path.join(HERE, "gqloc_cases.json")
FULL_STDOUT = 1500  # bytes kept verbatim
LIST_K = 11
BUILT = ("long_k16", "big_k25")


def rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def bases(data: bytes, skip_lines=1):
    """the sequence lines of a one-sequence FastA text, joined"""
    return "".join(data.decode().split("\n")[skip_lines:])


def main():
    for b in (REF, REF_MAKER):
        if not os.path.exists(b):
            sys.exit("build the reference first: make -C oracle ref")
    gcases, gfiles = G.load()
    by_id = {c["id"]: c for c in gcases["cases"]}
    work = tempfile.mkdtemp(prefix="gt4gqloc_")
    for name in gcases["files"]:
        with open(os.path.join(work, name), "wb") as fh:
            fh.write(G.file_bytes(gcases, name))
    for cid, data in gfiles.items():
        with open(os.path.join(work, by_id[cid]["output"]), "wb") as fh:
            fh.write(data)
    for cid in BUILT:
        p = subprocess.run([REF_MAKER] + by_id[cid]["argv"], cwd=work, capture_output=True, timeout=600)
        assert p.returncode == 0, (cid, p.stderr)
    files, lists = {}, {}

    def add_file(name, text):
        files[name] = text
        with open(os.path.join(work, name), "wb") as fh:
            fh.write(text.encode("latin-1"))

    # words of multi.fa at k = 11: FWD is its own canonical form, REV's canonical form is FWD; TWO is canonical, ABSENT in no text
    fwd, two, third, absent = "ACGTTGCAAGG", "AAGGCTTAACC", "GGATCCTTAAG", "AAAAAAAAAAC"
    rev = rc(fwd)
    assert M.canonical(M.string_to_word(fwd, 11), 11) == M.string_to_word(fwd, 11) and M.canonical(M.string_to_word(two, 11), 11) == M.string_to_word(two, 11)
    add_file("q_rev_fwd.txt", "\n".join([two, rev, fwd, absent, two, rc(third)]) + "\n")       # forward, then everything behind the reverse one prints 1
    add_file("q_fwd_rev.txt", "\n".join([fwd, absent, third, rc(two), two, fwd]) + "\n")
    add_file("q_fwd_only.txt", "\n".join([fwd, two, absent, third]) + "\n")                      # the flag never rises
    add_file("q_long.txt", "\n".join(["TT" + fwd + "CA", rev + "ACG", "GG" + two + "T"]) + "\n")
    qw = sorted({M.canonical(M.string_to_word(s, 11), 11) for s in (fwd, two, third, absent, "TTGACCAGGTA", "ACGTACGTACG")})
    lists["Q11"] = [[int(w), 7 + i] for i, w in enumerate(qw)]                                   # counts the index does not have: the zipper prints them
    write_list(os.path.join(work, "Q11.list"), make_records(np.array(qw, dtype=np.uint64), np.array([c for _, c in lists["Q11"]], dtype=np.uint32)), LIST_K)
    long_text = bases(G.file_bytes(gcases, "long.fa"))
    add_file("reads_long.fa", ">a piece of long.fa\n" + long_text[5000:5515] + "\n>and its reverse complement, one base changed\n" + rc(long_text[9000:9250] + "A" + long_text[9251:9500]) + "\n")
    big_text = "".join(l for l in G.file_bytes(gcases, "big.fa").decode().split("\n") if not l.startswith(">"))
    add_file("reads_big.fa", "".join(">r%d\n%s\n" % (i, big_text[p:p + 150] if i % 2 else rc(big_text[p:p + 150])) for i, p in enumerate(range(1000, 130000, 16000))))

    cases = []

    def ix(cid):
        return by_id[cid]["output"]

    def run(cid, argv, keep_stderr=False):
        p = subprocess.run([REF] + argv, cwd=work, capture_output=True, timeout=600)
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

    def query(cid, argv):
        assert "--locations" in argv
        run(cid, argv)
        run(cid + "_plain", [a for a in argv if a != "--locations"])

    # --files / --sequences: file I/O on the mapping
    for cid in ("multi_k11", "reads_k11", "two_files_k16", "three_files_k11", "long_name_k11", "many_k11", "crlf_k11", "nofinal_k11", "multi_c2_k2"):
        run("files_" + cid, [ix(cid), "--files"])
        run("sequences_" + cid, [ix(cid), "--sequences"])
    run("files_two_indexes_err", [ix("multi_k11"), ix("reads_k11"), "--files"], True)
    run("sequences_two_indexes_err", [ix("multi_k11"), ix("reads_k11"), "--sequences"], True)
    run("files_list_err", ["Q11.list", "--files"], True)
    run("sequences_list_err", ["Q11.list", "--sequences"], True)
    run("files_index_and_list_err", [ix("multi_k11"), "Q11.list", "--files"], True)
    run("sequences_with_query_list", [ix("multi_k11"), "-l", "Q11.list", "--sequences"])
    # the whole index with its locations
    for cid in ("multi_k1", "multi_k11", "multi_k32", "reads_k11", "lowc_k11", "lowc_c2_k11", "lowc_max3_k11", "lowc_c2_max3_k11", "three_files_k11", "many_k11"):
        run("dump_" + cid, [ix(cid), "--locations"])
    # -q
    for name, q in (("fwd", fwd), ("rev", rev), ("absent", absent), ("two", two)):
        query("q_" + name, [ix("multi_k11"), "-q", q, "--locations"])
    query("q_absent_min1", [ix("multi_k11"), "-q", absent, "--locations", "-min", "1"])
    query("q_fwd_min_max_ignored", [ix("multi_k11"), "-q", fwd, "--locations", "-min", "100", "-max", "1"])
    query("q_rev_mm1", [ix("three_files_k11"), "-q", rev, "--locations", "-mm", "1"])
    query("q_fwd_mm2_all", [ix("three_files_k11"), "-q", fwd, "--locations", "-mm", "2", "--all"])
    query("q_polya", [ix("lowc_k11"), "-q", "TTTTTTTTTTT", "--locations"])
    query("q_polya_mm1", [ix("lowc_k11"), "-q", "AAAAAAAAAAA", "--locations", "-mm", "1"])
    # -f: the sticky flag both ways
    for f in ("q_rev_fwd", "q_fwd_rev", "q_fwd_only"):
        query("f_%s_mm0" % f, [ix("three_files_k11"), "-f", f + ".txt", "--locations"])
        query("f_%s_mm1" % f, [ix("three_files_k11"), "-f", f + ".txt", "--locations", "-mm", "1"])
        query("f_%s_mm2_p3" % f, [ix("three_files_k11"), "-f", f + ".txt", "--locations", "-mm", "2", "-p", "3"])
    query("f_long_3p", [ix("multi_k11"), "-f", "q_long.txt", "--locations", "--3p"])
    query("f_long_5p_mm1", [ix("multi_k11"), "-f", "q_long.txt", "--locations", "--5p", "-mm", "1"])
    query("f_min1", [ix("multi_k11"), "-f", "q_fwd_rev.txt", "--locations", "-min", "1"])
    # -s
    query("s_reads_fq", [ix("three_files_k11"), "-s", "reads.fq", "--locations"])
    query("s_reads_fq_mm1", [ix("multi_k11"), "-s", "reads.fq", "--locations", "-mm", "1", "-min", "1"])
    query("s_second_fa", [ix("three_files_k11"), "-s", "second.fa", "--locations", "-min", "1"])
    # -l: the zipper prints the QUERY's count and REVERSE 0; with mismatches every word goes through search_one_word
    query("l_list_mm0", [ix("multi_k11"), "-l", "Q11.list", "--locations"])
    query("l_list_mm1", [ix("multi_k11"), "-l", "Q11.list", "--locations", "-mm", "1"])
    query("l_index_mm0", [ix("three_files_k11"), "-l", ix("multi_k11"), "--locations"])
    query("l_index_mm1", [ix("multi_k11"), "-l", ix("reads_k11"), "--locations", "-mm", "1", "-min", "1"])
    query("l_list_mm0_p2", [ix("multi_k11"), "-l", "Q11.list", "--locations", "-p", "2"])
    # larger, on indexes a replay builds itself
    query("big_s_long_k16", [ix("long_k16"), "-s", "reads_long.fa", "--locations"])
    query("big_s_long_k16_mm1", [ix("long_k16"), "-s", "reads_long.fa", "--locations", "-mm", "1", "-min", "1"])
    query("big_s_big_k25", [ix("big_k25"), "-s", "reads_big.fa", "--locations"])
    query("big_s_big_k25_mm1", [ix("big_k25"), "-s", "reads_big.fa", "--locations", "-mm", "1", "-min", "1"])

    shutil.rmtree(work, ignore_errors=True)
    with open(OUT, "w") as fh:
        json.dump(dict(files=files, lists=lists, built=list(BUILT), cases=cases), fh, indent=0, sort_keys=True)
    print("%d cases, %d bytes" % (len(cases), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
