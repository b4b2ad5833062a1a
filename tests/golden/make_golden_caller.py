#!/usr/bin/env python3
"""Golden transcripts of the reference's gmer_caller (reference src/gmer_caller.c) for genometester4_amd/gmer_caller and
tests/caller_model.py: argv, exit code, stdout, the stderr lines that do not depend on -D, and the "Iteration N delta V"
lines of -D -D.

The reference binary is taken from GT4_REF_GMER_CALLER, or compiled into a temporary directory from the reference tree
(REF, default /root/reference): the sources GMER_CALLER_SOURCES of its Makefile names, with the flags of oracle/Makefile
(REF_CFLAGS, REF_LIBS), as make_golden_gmer.py compiles gmer_counter.  Writes tests/golden/caller_cases.json:

    files    {name: text (latin-1) | {kind: markers, ...}: caller_util.markers}
    cases    [{id, argv, exit, stdout | stdout_sha256 + stdout_bytes, stderr_lines, iterations, device, trained, markers}]
    pipeline {argv, stdout ...}: the reference caller on the reference gmer_counter's output for gmer_util.big_reads /
             big_db with the nodes renamed "1:<n>" (--model full reads only lines that start with 1-9, X or Y)

What is kept: a trained case only if the reference prints the same bytes at --num_threads 1, 2, 3 and 16 (the chunks'
sums are then added in four different orders: a sum added in yet another order, on a GPU, is as likely to leave the output
alone); any case only if tests/caller_model.py replays it byte for byte and puts no printed probability within 1e-9 of
a value where %.2f rounds the other way.  At least 40 cases, 12 of them trained, must remain.  Kept out, because the
reference misbehaves and the drop-in refuses the input: their transcripts are the drop-in's own (tests/test_caller_cli.py)."""
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import caller_model as M  # noqa: E402
import caller_util as U  # noqa: E402
import gmer_util as GU  # noqa: E402
import make_golden_gmer as GG  # noqa: E402

THREADS = ("1", "2", "3", "16")


def reference_binary(tmp):
    given = os.environ.get("GT4_REF_GMER_CALLER")
    if given:
        return given
    src = os.path.join(os.environ.get("REF", "/root/reference"), "src")
    if not os.path.isdir(src):
        sys.exit("set GT4_REF_GMER_CALLER, or REF to the reference tree")
    mk = open(os.path.join(src, "Makefile")).read().replace("\\\n", " ")
    sources = [f for f in re.search(r"^GMER_CALLER_SOURCES =(.*)$", mk, re.M).group(1).split() if f.endswith(".c")]
    mk = open(os.path.join(ROOT, "oracle", "Makefile")).read().replace("\\\n", " ")
    cflags = re.search(r"^REF_CFLAGS := (.*)$", mk, re.M).group(1).replace("$(S)", src).split()
    libs = re.search(r"^REF_LIBS := (.*)$", mk, re.M).group(1).split()
    out = os.path.join(tmp, "gmer_caller")
    subprocess.check_call([os.environ.get("CC", "gcc")] + cflags + [os.path.join(src, f) for f in sources] + ["-o", out] + libs)
    return out


def near_boundary(v):
    """v lies within 1e-9 of k / 100 + 0.005: where %.2f turns from one value to the next"""
    if v != v or abs(v) == float("inf"):
        return False
    x = v * 100
    return abs(x - round(x - 0.5) - 0.5) < 1e-7


def texts():
    f = {}
    f["fem.txt"] = dict(kind="markers", seed=11, n_auto=400, n_x=60, n_y=30, coverage=30.0, male=False)
    f["male.txt"] = dict(kind="markers", seed=12, n_auto=400, n_x=60, n_y=30, coverage=30.0, male=True)
    f["auto.txt"] = dict(kind="markers", seed=13, n_auto=300, coverage=20.0)
    f["auto2.txt"] = dict(kind="markers", seed=14, n_auto=450, coverage=42.0, maf=0.2)
    f["pairs2.txt"] = dict(kind="markers", seed=15, n_auto=300, n_x=40, n_y=20, coverage=24.0, male=True, pairs=2)
    f["pairs3.txt"] = dict(kind="markers", seed=16, n_auto=300, n_x=40, n_y=20, coverage=24.0, male=False, pairs=3)
    f["big_f.txt"] = dict(kind="markers", seed=17, n_auto=5800, n_x=450, n_y=150, coverage=30.0, male=False)
    f["big_m.txt"] = dict(kind="markers", seed=18, n_auto=5800, n_x=450, n_y=150, coverage=30.0, male=True)
    # a marker without counts, counts at and above the log-factorial table, a marker whose likelihoods are all NaN, lines
    # --model full ignores (no digit 1-9, X or Y in front), CR LF, a line of 5 tokens and one of 9
    f["edge.txt"] = ("#gmer_counter version 4.2.16 (stable)\n#TextDatabase\tdb.txt\n"
                     "1:100\t2\t15\t17\n1:200\t2\t0\t0\n2:300\t2\t16383\t2\n2:400\t2\t3\t16384\n3:500\t2\t16390\t16390\n4:600\t2\t40000\t1\n"
                     "5:700\t2\t31\t0\n6:800\t2\t0\t29\n7:900\t3\t14\t15\t99\n8:1000\t8\t1\t2\t3\t4\t14\t16\t200\t300\n9:1100\t2\t30\t1\r\n"
                     "0:5\t2\t30\t30\nchr1:7\t2\t30\t30\nMT:9\t2\t30\t30\n\nx:11\t2\t30\t30\n"
                     "X:7\t2\t17000\t3\nX:8\t2\t14\t0\nX:9\t2\t13\t16\nY:1\t2\t0\t0\nY:2\t2\t1\t0\n")
    f["three.txt"] = "1:1\t2\t30\t0\n1:2\t2\t14\t16\n1:3\t2\t0\t31\n"
    return f


def main():
    t0 = time.time()
    tmp = tempfile.mkdtemp(prefix="gt4caller_ref_")
    ref = reference_binary(tmp)
    files = texts()
    doc = dict(files=files, cases=[])
    work = U.make_workdir(doc)
    cases, dropped = doc["cases"], []

    def run_ref(argv, cwd=work):
        p = subprocess.run([ref] + argv, cwd=cwd, capture_output=True, timeout=600)
        assert p.returncode >= 0, (argv, p.returncode, p.stderr[-300:])  # no crash transcripts
        return p

    def transcript(p, c):
        if len(p.stdout) <= U.FULL_STDOUT:
            c["stdout"] = p.stdout.decode("latin-1")
        else:
            c.update(stdout_sha256=U.sha(p.stdout), stdout_bytes=len(p.stdout))

    def run(cid, argv, name, trained=False, device=True):
        """argv without the file; a trained case runs with -D -D"""
        assert cid not in [x["id"] for x in cases], cid
        text = U.file_bytes(doc, name) if name else b""
        full = argv + (["-D", "-D"] if trained else []) + ([name] if name else [])
        p = run_ref(full)
        if trained:
            for n in THREADS:
                q = run_ref(argv + ["--num_threads", n, name])
                if q.stdout != p.stdout or q.returncode != p.returncode:
                    dropped.append((cid, "differs at --num_threads " + n))
                    return
        err = p.stderr.decode("latin-1")
        c = dict(id=cid, argv=full, exit=p.returncode, device=device, trained=trained, markers=text.count(b"\n"), iterations=U.iterations(p.stderr),
                 stderr_lines=[l for l in err.split("\n") if l.startswith("Y inconsistency") or l.startswith("No calls")])
        transcript(p, c)
        if device:
            m = M.run_cli(full, text)
            if (m.exit, m.stdout) != (p.returncode, p.stdout):
                dropped.append((cid, "the model prints something else"))
                return
            assert m.stderr_lines == c["stderr_lines"] and (not trained or m.iterations == c["iterations"]), cid
            near = [v for v in m.printed if near_boundary(v)]
            if near:
                dropped.append((cid, "a probability within 1e-9 of a rounding boundary: %r" % near[0]))
                return
        else:
            c["stderr"] = err
        cases.append(c)

    # --runs 0: the three models, the output switches, both sexes, lines of 2 and 3 pairs, the edge markers
    for name, cov in (("fem.txt", "30"), ("male.txt", "30"), ("pairs2.txt", "24"), ("pairs3.txt", "24"), ("edge.txt", "20")):
        stem = name.split(".")[0]
        run("r0_%s_cov" % stem, ["--runs", "0", "--coverage", cov], name)
        run("r0_%s_alt_header_info" % stem, ["--runs", "0", "--coverage", cov, "--alternatives", "--header", "--info"], name)
        run("r0_%s_nc_cutoff" % stem, ["--runs", "0", "--coverage", cov, "--non_canonical", "--prob_cutoff", "0.99"], name)
    run("r0_fem_no_coverage_all_nc", ["--runs", "0"], "fem.txt")
    run("r0_fem_no_coverage_alt", ["--runs", "0", "--alternatives", "--info"], "fem.txt")
    run("r0_male_params", ["--runs", "0", "--params", "0.05", "0.0001", "0.02", "0.97", "28", "60", "-0.5", "--alternatives"], "male.txt")
    run("r0_male_params_lisa_negative", ["--runs", "0", "--params", "0.05", "0.1", "0.3", "0.7", "28", "60", "-0.5", "--alternatives"], "male.txt")
    run("r0_male_params_size_nonpositive", ["--runs", "0", "--params", "0.05", "0.0001", "0.02", "0.97", "30", "20", "-0.5", "--alternatives"], "male.txt")
    run("r0_edge_diploid_header_only", ["--runs", "0", "--coverage", "20", "--model", "diploid", "--no_genotypes", "--header", "--info"], "three.txt")
    run("r0_auto_diploid", ["--runs", "0", "--coverage", "20", "--model", "diploid", "--alternatives"], "auto.txt")
    run("r0_auto_haploid", ["--runs", "0", "--coverage", "20", "--model", "haploid", "--alternatives", "--info"], "auto.txt")
    run("r0_auto_haploid_nc", ["--runs", "0", "--coverage", "40", "--model", "haploid", "--non_canonical"], "auto.txt")
    run("r0_auto2_diploid_cutoff", ["--runs", "0", "--coverage", "42", "--model", "diploid", "--prob_cutoff", "0.99", "--header"], "auto2.txt")
    run("r0_no_genotypes_info", ["--runs", "0", "--coverage", "30", "--no_genotypes", "--info"], "male.txt")
    run("r0_threads_ignored", ["--runs", "0", "--coverage", "30", "--num_threads", "3", "--training_size", "10"], "fem.txt")
    run("r0_big_f", ["--runs", "0", "--coverage", "30", "--info"], "big_f.txt")
    run("r0_big_m_alt", ["--runs", "0", "--coverage", "30", "--alternatives"], "big_m.txt")
    # trained
    run("t_fem", ["--info"], "fem.txt", trained=True)
    run("t_male", ["--info", "--alternatives"], "male.txt", trained=True)
    run("t_male_runs1", ["--runs", "1", "--info"], "male.txt", trained=True)
    run("t_fem_runs2_header", ["--runs", "2", "--header", "--info"], "fem.txt", trained=True)
    run("t_fem_coverage", ["--runs", "1", "--coverage", "27", "--info"], "fem.txt", trained=True)
    run("t_male_params", ["--runs", "1", "--params", "0.05", "0.0001", "0.02", "0.97", "28", "60", "-0.5", "--info"], "male.txt", trained=True)
    run("t_auto_diploid", ["--model", "diploid", "--runs", "2", "--info"], "auto.txt", trained=True)
    run("t_auto_haploid", ["--model", "haploid", "--runs", "2", "--info", "--non_canonical"], "auto.txt", trained=True)
    run("t_auto2_diploid", ["--model", "diploid", "--runs", "3", "--info", "--prob_cutoff", "0.99"], "auto2.txt", trained=True)
    run("t_auto2_training_size", ["--model", "diploid", "--runs", "1", "--training_size", "200", "--info"], "auto2.txt", trained=True)
    run("t_pairs2", ["--runs", "1", "--info"], "pairs2.txt", trained=True)
    run("t_pairs3", ["--runs", "1", "--info", "--alternatives"], "pairs3.txt", trained=True)
    run("t_pairs2_no_genotypes", ["--runs", "2", "--info", "--no_genotypes"], "pairs2.txt", trained=True)
    run("t_auto_full_model", ["--runs", "1", "--info"], "auto.txt", trained=True)
    run("t_three_degenerate", ["--model", "diploid", "--runs", "1", "--info"], "three.txt", trained=True)
    run("t_big_f", ["--info"], "big_f.txt", trained=True)
    run("t_big_m", ["--info"], "big_m.txt", trained=True)
    # no device: -v, usage errors, files that cannot be read
    run("version", ["-v"], None, device=False)
    run("version_long", ["--runs", "0", "--version"], None, device=False)
    run("err_no_file", [], None, device=False)
    run("err_missing_file", ["nothere.txt"], None, device=False)
    for opt in ("--runs", "--training_size", "--num_threads", "--prob_cutoff", "--model", "--coverage", "--params"):
        run("err_last_%s" % opt.strip("-"), ["fem.txt", opt], None, device=False)
    run("err_params_six", ["--params", "1", "2", "3", "4", "5", "6"], None, device=False)
    run("err_model_unknown", ["--model", "triploid", "fem.txt"], None, device=False)
    run("err_two_files", ["fem.txt", "male.txt"], None, device=False)

    # the pipeline: gmer_counter's output into gmer_caller
    pdir = tempfile.mkdtemp(prefix="gt4caller_pipe_")
    with open(os.path.join(pdir, "db.txt"), "wb") as f:
        f.write(U.pipeline_db())
    with open(os.path.join(pdir, "reads.fq"), "wb") as f:
        f.write(GU.big_reads())
    counter = GG.reference_binary(tmp)
    counts = subprocess.run([counter, "-db", "db.txt", "reads.fq"], cwd=pdir, capture_output=True, check=True).stdout
    with open(os.path.join(pdir, "counts.txt"), "wb") as f:
        f.write(counts)
    argv = ["--runs", "0", "--coverage", "15", "--alternatives", "--info", "counts.txt"]
    p = run_ref(argv, cwd=pdir)
    m = M.run_cli(argv, counts)
    assert (m.exit, m.stdout) == (p.returncode, p.stdout) and p.returncode == 0 and len(p.stdout) > 10000
    assert not [v for v in m.printed if near_boundary(v)]
    doc["pipeline"] = dict(argv=argv, exit=0, counts_sha256=U.sha(counts), counts_bytes=len(counts))
    transcript(p, doc["pipeline"])

    shutil.rmtree(work, ignore_errors=True)
    shutil.rmtree(pdir, ignore_errors=True)
    shutil.rmtree(tmp, ignore_errors=True)
    for d in dropped:
        print("dropped: %s: %s" % d)
    trained = [c for c in cases if c["trained"]]
    assert len(cases) >= 40 and len(trained) >= 12, (len(cases), len(trained))
    assert sum(1 for c in trained if c["markers"] <= 3) <= 1
    with open(U.CASES_PATH, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
    print("%d cases (%d trained, %d dropped), %d bytes, %.1f s" % (len(cases), len(trained), len(dropped), os.path.getsize(U.CASES_PATH), time.time() - t0))


if __name__ == "__main__":
    main()
