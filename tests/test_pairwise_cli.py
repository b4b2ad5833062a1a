"""glistcompare L1 .. LN --pairwise: what every list shares with every other one, on stdout.

Without a device: every message and exit code the option has before any device is opened, and -h as the reference prints it.
On the GPU: every case of tests/golden/pairwise_cases.json (the numbers the reference binary printed for every pair of lists,
tests/golden/make_golden_pairwise.py) through the binary, byte for byte; the file names as given; -D, --stream and
--disable_scouts."""
import os
import shutil
import subprocess
import tempfile

import pytest

import golden_util as G
import pairwise_util as PU
from genometester4_amd.listio import write_list

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "genometester4_amd", "glistcompare")
CASES = PU.load_golden()
REF_HELP = next(c for c in G.load()[0] if c["tool"] == "glistcompare" and c["id"] == "help")
TIMEOUT = 120
HEADER = "#I\tJ\tLIST_I\tLIST_J\tSHARED\tMIN_TOTAL\tUNION\tJACCARD\n"


def _env(**extra):
    return dict({k: v for k, v in os.environ.items() if not k.startswith("GT4HIP_")}, **extra)


def _files(case, prefix=""):
    return ["%s%s_%d.list" % (prefix, case["id"], j) for j in range(len(case["records"]))]


@pytest.fixture(scope="module")
def work():
    """the lists of the goldens as <case>_<j>.list, and once more under sub/"""
    d = tempfile.mkdtemp(prefix="gt4pw_cli_")
    os.mkdir(os.path.join(d, "sub"))
    for case in CASES:
        for prefix in ("", "sub/"):
            for name, rec in zip(_files(case, prefix), case["records"]):
                write_list(os.path.join(d, name), rec, case["word_length"])
    yield d
    shutil.rmtree(d, ignore_errors=True)


def _run(argv, cwd, env=None, cli=CLI):
    """(exit, stdout, stderr, names of the files the run left, which are removed)"""
    before = set(os.listdir(cwd))
    p = subprocess.run([cli] + argv, cwd=cwd, capture_output=True, timeout=TIMEOUT, env=env or _env())
    left = sorted(set(os.listdir(cwd)) - before)
    for f in left:
        os.remove(os.path.join(cwd, f))
    return p.returncode, p.stdout.decode("latin-1"), p.stderr.decode("latin-1"), left


def _expected(case, names):
    """the transcript, every number of it one the reference printed"""
    n = len(names)
    diag = {d["i"]: d["intersection"] for d in case["diagonal"]}
    pair = {(p["i"], p["j"]): p for p in case["pairs"]}
    out = [HEADER]
    for i in range(n):
        for j in range(i, n):
            if i == j:
                shared, total = diag[i]
                union = shared
            else:
                shared, total = pair[i, j]["intersection"]
                union = pair[i, j]["union"][0]
            out.append("%d\t%d\t%s\t%s\t%d\t%d\t%d\t%.6f\n" % (i, j, names[i], names[j], shared, total, union, shared / union if union else 0.0))
    return "".join(out)


# ------------------------------------------------------------------ decided before any device is opened

A3 = ["k1_n3_0.list", "k1_n3_1.list", "k1_n3_2.list"]
COMBINED = "Error: --pairwise compares every list with every other one by itself: it cannot be combined with %s\n"
REFUSED = [
    (A3 + ["--pairwise", "-u"], COMBINED % "-u"),
    (A3 + ["-i", "--pairwise"], COMBINED % "-i"),
    (A3[:2] + ["--pairwise", "-d"], COMBINED % "-d"),
    (A3[:2] + ["--pairwise", "-dd"], COMBINED % "-dd"),
    (A3[:2] + ["--pairwise", "-du"], COMBINED % "-du"),
    (A3[:2] + ["--pairwise", "-mm", "1"], COMBINED % "-mm"),
    (A3[:1] + ["--subset", "rand", "5", "--pairwise"], COMBINED % "--subset"),
    (A3 + ["--pairwise", "--min_lists", "2"], COMBINED % "--min_lists / --max_lists"),
    (A3 + ["--pairwise", "--max_lists", "2"], COMBINED % "--min_lists / --max_lists"),
    (A3 + ["--pairwise", "-r", "max"], COMBINED % "-r"),
    (A3 + ["--pairwise", "-r", "default"], COMBINED % "-r"),
    (A3 + ["--pairwise", "-c", "2"], COMBINED % "-c"),
    (A3 + ["--pairwise", "-c", "1"], COMBINED % "-c"),
    (A3 + ["--pairwise", "--count_cutoff", "2"], COMBINED % "-c"),
    (A3 + ["--pairwise", "--count_only"], COMBINED % "--count_only"),
    (A3 + ["--pairwise", "--gpus", "2"], COMBINED % "--gpus"),
    (A3 + ["--pairwise", "--gpus", "1"], COMBINED % "--gpus"),
    (A3[:1] + ["--pairwise"], "Error: At least 2 list/index files are needed\n"),
    (["--pairwise"], "Error: At least 2 list/index files are needed\n"),
]


@pytest.mark.parametrize("argv,message", REFUSED, ids=["%d files %s" % (sum(x.endswith(".list") for x in a), " ".join(x for x in a if not x.endswith(".list"))) for a, _ in REFUSED])
def test_refused_before_any_device_is_opened(argv, message, work):
    # (a device that does not exist: whoever opened one would say so instead)
    code, out, err, left = _run(argv, work, _env(GT4HIP_DEVICE="1000", HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES=""))
    assert (code, out, err, left) == (1, "", message, [])


@pytest.mark.parametrize("env,what", [({"GT4HIP_HBM_LIMIT": "4K"}, "GT4HIP_HBM_LIMIT"), ({"GT4HIP_GPUS": "2"}, "GT4HIP_GPUS")])
def test_chunks_and_worker_processes_are_refused(env, what, work):
    code, out, err, left = _run(A3 + ["--pairwise"], work, _env(GT4HIP_DEVICE="1000", HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", **env))
    assert (code, out, err, left) == (1, "", "Error: --pairwise needs all lists resident on one GPU: it cannot be combined with %s\n" % what, [])


def test_help_is_the_reference_transcript(work):
    code, out, err, left = _run(["-h"], work)
    assert (code, out, err, left) == (REF_HELP["exit"], REF_HELP["stdout"], REF_HELP["stderr"], [])
    assert "pairwise" not in out


def test_a_build_without_the_entry_point_says_so(work):
    """tests/harness links the command line against a CPU stand-in that has no gt4hip_pairwise_multi: the weak symbol is
    absent, and the option is an error behind its own checks"""
    harness = os.path.join(ROOT, "tests", "harness")
    r = subprocess.run(["make", "-C", harness, "_build/glistcompare_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    stub = os.path.join(harness, "_build", "glistcompare_asan")
    assert _run(A3 + ["--pairwise"], work, cli=stub) == (1, "", "Error: this build has no --pairwise path\n", [])
    assert _run(A3 + ["--pairwise", "-u"], work, cli=stub) == (1, "", COMBINED % "-u", [])


# ------------------------------------------------------------------ on the GPU

@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_golden_through_the_binary(case, work):
    names = _files(case)
    assert _run(names + ["--pairwise"], work) == (0, _expected(case, names), "", [])


@pytest.mark.gpu
def test_names_as_given_and_options_that_add_nothing(work):
    case = next(c for c in CASES if c["id"] == "k25_n5_shapes")
    names = _files(case, "sub/")[:2] + ["./" + f for f in _files(case)[2:]]
    want = _expected(case, names)
    assert want.count("\n") == 1 + 15 and "\t0\t0\t0\t0.000000\n" in want and "\t1.000000\n" in want
    assert _run(["--pairwise"] + names, work) == (0, want, "", [])
    assert _run(names + ["--pairwise", "--stream", "--disable_scouts", "-o", "unused"], work) == (0, want, "", [])
    assert _run(names + ["--pairwise", "-D"], work) == (0, want, "Rule: 0\nNum files: 5\n", [])
