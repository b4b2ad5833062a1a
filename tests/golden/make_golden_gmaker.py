#!/usr/bin/env python3
"""Golden transcripts of the reference's glistmaker (reference src/glistmaker.c:138-353) for genometester4_amd/glistmaker
and tests/maker_model.py: argv, exit code, stdout, stderr and the bytes (or SHA-256) of the .list file it wrote.

Needs oracle/_ref/glistmaker (make -C oracle ref).  Writes tests/golden/gmaker_cases.json:

    files    {name: text (latin-1) | {seed, n_bases}: gmaker_util.big_fasta}
    cases    [{id, argv, exit, stdout, stderr, output: name of the file written | null, list_hex | list_sha256 + list_bytes}]

Every case whose list is compared is one where the reference ends with exit 0.  Kept out, because the reference does
not behave deterministically (or not usefully) there:
  * what it leaves behind after a reader error (bad start tag, FastQ without '+'): it carries on reading behind the
    error, one message per byte for a bad start tag, and writes what it still finds; the cases keep the transcript's
    first stderr line and no list;
  * a name above 200 characters for -o ends without a newline on stderr and exit 1: kept (deterministic);
  * standard input ('-') depends on the stream reader's buffering of the caller's pipe: not recorded."""
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gmaker_util as U  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "glistmaker")
FULL_LIST = 2000  # bytes of a list kept verbatim (hex)


def texts():
    f = {}
    f["multi.fa"] = (">one first sequence\nACGTTGCAAGGCTTAACCGGTTAAGGCCTTAGCTAGCTAGGATCCGATCGATTACGCGCGATATCG\nGGATCCTTAAGGCCAATTGGCCAATTCCGG\nacgtuuacgguacgtUUACG\n"
                     ">two\nACGTNNNNNNACGTACGTACGTTTGACCANACGTAGCTAGCTAGGCTAGCTAGGATCGATCGGCTAGCTAGCTA\n>three mid>line\nACGTACGGTAC>GTA in a name ACGTACGTACGTACGTACGTACGTACGTACGTACGT\nTTGACCAGGTACCAGTTGACCAGGTACCAGTTGACCAGGTAC\n")
    f["crlf.fa"] = ">crlf one\r\nACGTTGCAAGGCTTAACCGGTTAAGGCC\r\nTTAGCTAGCTAGGATCCGATCGATTACGCGCGATATCG\r\n>crlf two\r\nGGATCCTTAAGGCCAATTGGCC\tAATTCCGG\r\n"
    f["nofinal.fa"] = ">no final newline\nACGTTGCAAGGCTTAACCGGTTAAGGCCTTAGCTAGCTAGGATCCGATCG\nATTACGCGCGATATCGGGATCCTTAAGG"
    f["empty_seq.fa"] = ">empty\n>also empty\n\n>short\nACGTA\n>long enough\nACGTTGCAAGGCTTAACCGGTTAAGGCCTTAGCTAGCTAGGATCCGATCGATTACGCG\n"
    f["reads.fq"] = ("@r1 first\nACGTTGCAAGGCTTAACCGGTTAAGGCCTTAGCTAGCTAGG\n+\n@IIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n"
                     "@r2\nGGATCCTTAAGGCCAATTGGNCAATTCCGGACGTACGTAA\n+r2 again\n>III+IIIIIIIIIIII@IIIIIIIIIIIIIIIIIIIIII\n"
                     "@r3 with > in sequence\nACGTTGCAAGGCTTAACC>GGTTAAGGCCTTAGCTAGCTAGGATCCGATCGATTACGCGCGATATCG\n+\n+III@III>IIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n")
    f["second.fa"] = ">second file\nTTAGCTAGCTAGGATCCGATCGATTACGCGCGATATCGACGTTGCAAGGCTTAACCGGTTAAGGCC\nACGTACGTACGTACGTACGTACGTACGTACGTACGTAC\n"
    f["big.fa"] = dict(seed=4242, n_bases=130_000)
    f["bad_start.fa"] = "ACGT\n>x\nACGTACGTACGT\n"
    f["no_plus.fq"] = "@r1\nACGTTGCAAGGCTTAACCGG\nIIIIIIIIIIIIIIIIIIII\n@r2\nACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIII\n"
    return f


def main():
    if not os.path.exists(REF):
        sys.exit("build the reference first: make -C oracle ref")
    t0 = time.time()
    files = texts()
    cases_doc = dict(files=files, cases=[])
    work = U.make_workdir(cases_doc)
    cases = cases_doc["cases"]

    def run(cid, argv, output=None, keep_list=True, first_stderr_line_only=False):
        if output and os.path.exists(os.path.join(work, output)):
            os.remove(os.path.join(work, output))
        p = subprocess.run([REF] + argv, cwd=work, capture_output=True, timeout=300)
        assert p.returncode >= 0, (cid, p.returncode)  # no crash transcripts
        err = p.stderr.decode("latin-1")
        if first_stderr_line_only:
            err = err.split("\n")[0] + "\n"
        c = dict(id=cid, argv=argv, exit=p.returncode, stdout=p.stdout.decode("latin-1"), stderr=err, output=output if keep_list else None)
        if output and keep_list:
            assert p.returncode == 0, (cid, p.returncode, err)
            data = open(os.path.join(work, output), "rb").read()
            if len(data) <= FULL_LIST:
                c["list_hex"] = data.hex()
            else:
                c.update(list_sha256=U.sha(data), list_bytes=len(data))
        assert cid not in [x["id"] for x in cases], cid
        cases.append(c)

    for k in (1, 5, 16, 25, 31, 32):
        for name in ("multi.fa", "crlf.fa", "nofinal.fa", "empty_seq.fa", "reads.fq"):
            run("%s_k%d" % (name.replace(".", "_"), k), [name, "-w", str(k), "-o", "o"], "o_%d.list" % k)
    run("two_files_k16", ["multi.fa", "second.fa", "-w", "16", "-o", "two"], "two_16.list")
    run("three_files_k25", ["multi.fa", "reads.fq", "second.fa", "-w", "25", "-o", "three"], "three_25.list")
    run("out_in_dir_k16", ["multi.fa", "-w", "16", "-o", "dir/name"], "dir/name_16.list")
    run("default_out_k5", ["second.fa", "--wordlength", "5"], "out_5.list")
    run("cutoffs_k5", ["multi.fa", "-w", "5", "-c", "2", "--max", "3", "-o", "cut"], "cut_5.list")
    run("ignored_options_k16", ["multi.fa", "-w", "16", "-o", "ign", "--num_threads", "3", "--max_tables", "999", "--tmpdir", ".", "--stream"], "ign_16.list")
    run("table_size_swallows_k16", ["multi.fa", "-w", "16", "-o", "ts", "--table_size", "4096", "swallowed"], "ts_16.list")
    for k in (16, 25, 32):
        run("big_k%d" % k, ["big.fa", "-w", str(k), "-o", "big"], "big_%d.list" % k)
    # every argv error of :159-252, -v, -h, a missing file
    run("version", ["-v"])
    run("version_long", ["--version", "multi.fa"])
    run("help", ["-h"])
    run("help_q", ["multi.fa", "-?"])
    run("err_o_last", ["multi.fa", "-o"])
    run("err_w_last", ["multi.fa", "-w"])
    run("err_w_text", ["multi.fa", "-w", "16x"])
    run("err_c_last", ["multi.fa", "-w", "16", "-c"])
    run("err_c_text", ["multi.fa", "-w", "16", "--cutoff", "x"])
    run("err_max_last", ["multi.fa", "-w", "16", "--max"])
    run("err_max_text", ["multi.fa", "-w", "16", "--max", "1.5"])
    run("err_threads_last", ["multi.fa", "--num_threads"])
    run("err_threads_text", ["multi.fa", "-w", "16", "--num_threads", "many"])
    run("err_tables_last", ["multi.fa", "--max_tables"])
    run("err_tables_text", ["multi.fa", "-w", "16", "--max_tables", "x"])
    run("err_table_size_last", ["multi.fa", "--table_size"])
    run("err_table_size_text", ["multi.fa", "-w", "16", "--table_size", "1k"])
    run("err_tmpdir_last", ["multi.fa", "--tmpdir"])
    run("err_unknown", ["multi.fa", "-w", "16", "--nonsense"])
    run("err_no_file", ["-w", "16"])
    run("err_no_args", [])
    run("err_w_missing", ["multi.fa"])
    run("err_w_0", ["multi.fa", "-w", "0"])
    run("err_w_33", ["multi.fa", "-w", "33"])
    run("err_min_0", ["multi.fa", "-w", "16", "--min", "0"])
    run("err_range", ["multi.fa", "-w", "16", "-c", "5", "--max", "4"])
    run("err_long_name", ["multi.fa", "-w", "16", "-o", "n" * 201])
    run("err_missing_file", ["multi.fa", "nothere.fa", "-w", "16"])
    # reader errors: the first line of the transcript, no list (see the docstring)
    run("bad_start_k4", ["bad_start.fa", "-w", "4", "-o", "bad"], "bad_4.list", keep_list=False, first_stderr_line_only=True)
    run("no_plus_k4", ["no_plus.fq", "-w", "4", "-o", "bad"], "bad_4.list", keep_list=False, first_stderr_line_only=True)

    shutil.rmtree(work, ignore_errors=True)
    with open(U.CASES_PATH, "w") as f:
        json.dump(cases_doc, f, indent=0, sort_keys=True)
    print("%d cases, %d bytes, %.1f s" % (len(cases), os.path.getsize(U.CASES_PATH), time.time() - t0))


if __name__ == "__main__":
    main()
