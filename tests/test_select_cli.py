"""glistcompare L1 .. LN -u --min_lists M [--max_lists X]: the words of M to X of the N lists, with the union's counts.

Without a device: every message and exit code the options have before any device is opened, and -h as the reference
prints it.  On the GPU: every case of tests/golden/select_cases.json (expected records derived from outputs of the
reference binary alone, tests/golden/make_golden_select.py) through the binary, file bytes and all; --min_lists 1 against
the reference's own union files of tests/golden/cases.json; the same bytes from key-range chunks and from two worker
processes; --count_only."""
import os
import shutil
import subprocess
import tempfile

import pytest

import golden_util as G
import select_util as SU
from genometester4_amd.listio import header_bytes, write_list, write_list_v40

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "genometester4_amd", "glistcompare")
INPUTS, CASES = SU.load_golden()
REF_CASES, REF_INPUTS, REF_OUTPUTS = G.load()
REF_CASES = {c["id"]: c for c in REF_CASES if c["tool"] == "glistcompare"}
TIMEOUT = 120


def _env(**extra):
    return dict({k: v for k, v in os.environ.items() if not k.startswith("GT4HIP_")}, **extra)


@pytest.fixture(scope="module")
def work():
    """the lists of the select goldens as n<N>_<j>.list, and the inputs of tests/golden/cases.json under their names"""
    d = tempfile.mkdtemp(prefix="gt4sel_cli_")
    for name, (k, lists) in INPUTS.items():
        for j, rec in enumerate(lists):
            write_list(os.path.join(d, "%s_%d.list" % (name, j)), rec, k)
    for name, (rec, k, flavour) in REF_INPUTS.items():
        (write_list_v40 if flavour == "v40" else write_list)(os.path.join(d, name + ".list"), rec, k)
    yield d
    shutil.rmtree(d, ignore_errors=True)


def _run(argv, cwd, env=None):
    """(exit, stdout, stderr, {name: bytes} of the files the run left, which are removed)"""
    before = set(os.listdir(cwd))
    p = subprocess.run([CLI] + argv, cwd=cwd, capture_output=True, timeout=TIMEOUT, env=env or _env())
    left = {}
    for f in sorted(set(os.listdir(cwd)) - before):
        with open(os.path.join(cwd, f), "rb") as fh:
            left[f] = fh.read()
        os.remove(os.path.join(cwd, f))
    return p.returncode, p.stdout.decode("latin-1"), p.stderr.decode("latin-1"), left


def _files(name):
    return ["%s_%d.list" % (name, j) for j in range(len(INPUTS[name][1]))]


def _argv(case, out="s"):
    argv = _files(case["inputs"]) + ["-u", "--min_lists", str(case["min_lists"]), "--max_lists", str(case["max_lists"]), "-o", out]
    if case["rule"] != "default":
        argv += ["-r", case["rule"]]
    if case["cutoff"] != 1:
        argv += ["-c", str(case["cutoff"])]
    return argv


def _expected_file(case):
    k = INPUTS[case["inputs"]][0]
    name = "s_%d_select_%d_%d.list" % (k, case["min_lists"], case["max_lists"])
    return name, header_bytes(k, case["n_words"], case["total_count"]) + case["expected"].tobytes()


# ------------------------------------------------------------------ decided before any device is opened

A3 = ["n3_0.list", "n3_1.list", "n3_2.list"]
COMBINED = "Error: --min_lists / --max_lists select from the union of the lists: they cannot be combined with %s\n"
BOUNDS = "Error: --min_lists %d, --max_lists %d: 1 <= min_lists <= max_lists <= %d (the number of files) is needed\n"
REFUSED = [
    (A3 + ["--min_lists", "2"], "Error: --min_lists / --max_lists select from the union of the lists: -u is needed\n"),
    (A3 + ["--max_lists", "2"], "Error: --min_lists / --max_lists select from the union of the lists: -u is needed\n"),
    (A3 + ["-u", "-i", "--min_lists", "2"], COMBINED % "-i"),
    (A3[:2] + ["-u", "-d", "--min_lists", "2"], COMBINED % "-d"),
    (A3[:2] + ["-u", "-dd", "--max_lists", "1"], COMBINED % "-dd"),
    (A3[:2] + ["-u", "-du", "--min_lists", "2"], COMBINED % "-du"),
    (A3[:2] + ["-u", "-d", "-mm", "1", "--min_lists", "2"], COMBINED % "-mm"),
    (A3[:1] + ["--subset", "rand", "5", "-u", "--min_lists", "1"], COMBINED % "--subset"),
    (A3 + ["-u", "--min_lists", "x"], "Error: Invalid --min_lists: x! Must be an integer.\n"),
    (A3 + ["-u", "--min_lists", "2x"], "Error: Invalid --min_lists: 2x! Must be an integer.\n"),
    (A3 + ["-u", "--max_lists", "1.5"], "Error: Invalid --max_lists: 1.5! Must be an integer.\n"),
    (A3 + ["-u", "--max_lists", ""], "Error: Invalid --max_lists: ! Must be an integer.\n"),
    (A3 + ["-u", "--min_lists"], "Error: --min_lists needs a number of lists\n"),
    (A3 + ["-u", "--min_lists", "0"], BOUNDS % (0, 3, 3)),
    (A3 + ["-u", "--min_lists", "-1"], BOUNDS % (-1, 3, 3)),
    (A3 + ["-u", "--min_lists", "3", "--max_lists", "2"], BOUNDS % (3, 2, 3)),
    (A3 + ["-u", "--max_lists", "4"], BOUNDS % (1, 4, 3)),
    (A3 + ["-u", "--min_lists", "4"], BOUNDS % (4, 3, 3)),
    (A3[:2] + ["-u", "--max_lists", "3"], BOUNDS % (1, 3, 2)),
    (A3[:1] + ["-u", "--min_lists", "1"], "Error: At least 2 list/index files are needed\n"),
    (["-u", "--max_lists", "1"], "Error: At least 2 list/index files are needed\n"),
]


@pytest.mark.parametrize("argv,message", REFUSED, ids=["%d files %s" % (sum(x.endswith(".list") for x in a), " ".join(x for x in a if not x.endswith(".list"))) for a, _ in REFUSED])
def test_refused_before_any_device_is_opened(argv, message, work):
    # (a device that does not exist: whoever opened one would say so instead)
    code, out, err, left = _run(argv, work, _env(GT4HIP_DEVICE="1000", HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES=""))
    assert (code, out, err, left) == (1, "", message, {})


@pytest.mark.parametrize("rule,ref", [("min", "pair_only_u_r_min"), ("subtract", "pair_only_u_r_subtract"), ("first", None), ("second", None)])
def test_a_rule_the_union_refuses_gives_what_the_union_prints(rule, ref, work):
    plain = _run(A3 + ["-u", "-r", rule], work)
    code, out, err, left = _run(A3 + ["-u", "--min_lists", "2", "-r", rule], work)
    assert (code, out, err, left) == plain and code == 1 and err.startswith("Error: ") and not left
    if ref:
        assert err == REF_CASES[ref]["stderr"]


def test_help_is_the_reference_transcript(work):
    code, out, err, left = _run(["-h"], work)
    assert (code, out, err, left) == (REF_CASES["help"]["exit"], REF_CASES["help"]["stdout"], REF_CASES["help"]["stderr"], {})
    assert "min_lists" not in out


def test_a_build_without_the_entry_point_says_so(work):
    """tests/harness links the command line against a CPU stand-in that has no gt4hip_select_multi: the weak symbol is
    absent, and the options are an error behind their own checks"""
    harness = os.path.join(ROOT, "tests", "harness")
    r = subprocess.run(["make", "-C", harness, "_build/glistcompare_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    stub = os.path.join(harness, "_build", "glistcompare_asan")
    p = subprocess.run([stub] + A3 + ["-u", "--min_lists", "2"], cwd=work, capture_output=True, timeout=TIMEOUT, env=_env())
    assert (p.returncode, p.stdout, p.stderr) == (1, b"", b"Error: this build has no --min_lists / --max_lists path\n")
    p = subprocess.run([stub] + A3 + ["-u", "--min_lists", "4"], cwd=work, capture_output=True, timeout=TIMEOUT, env=_env())
    assert (p.returncode, p.stderr.decode()) == (1, BOUNDS % (4, 3, 3))


# ------------------------------------------------------------------ on the GPU

@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_golden_through_the_binary(case, work):
    code, out, err, left = _run(_argv(case), work)
    name, data = _expected_file(case)
    assert (code, out, err) == (0, "", "")
    assert sorted(left) == [name]
    assert left[name] == data


def _union_only(case):
    """a run of tests/golden/cases.json on three and more lists that wrote a union, over lists without a count of 0 (where
    every word of the union lies in at least one list)"""
    files = [a for a in case["argv"] if a.endswith(".list")]
    return (len(files) > 2 and case["exit"] == 0 and "-u" in case["argv"] and any(f.endswith("_union.list") for f in case["files"])
            and all(len(REF_INPUTS[f[:-5]][0]) == 0 or int(REF_INPUTS[f[:-5]][0]["count"].min()) >= 1 for f in files))


UNION_CASES = [c for c in REF_CASES.values() if _union_only(c)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", UNION_CASES, ids=[c["id"] for c in UNION_CASES])
def test_min_lists_1_is_the_union_of_the_reference(case, work):
    assert len(UNION_CASES) >= 10
    argv = [a for a in case["argv"] if a not in ("-i", "--count_only")] + ["--min_lists", "1"]
    n = sum(a.endswith(".list") for a in argv)
    union = next(f for f in case["files"] if f.endswith("_union.list"))
    code, out, err, left = _run(argv, work)
    assert (code, out, err) == (0, "", "")
    assert sorted(left) == [union.replace("_union.list", "_select_1_%d.list" % n)]
    assert list(left.values())[0] == bytes(REF_OUTPUTS["%s/%s" % (case["id"], union)])


LARGEST = max(CASES, key=lambda c: (len(INPUTS[c["inputs"]][1]), c["n_words"]))


@pytest.mark.gpu
def test_key_range_chunks_give_the_same_bytes(work):
    name, data = _expected_file(LARGEST)
    code, out, err, left = _run(_argv(LARGEST), work, _env(GT4HIP_HBM_LIMIT="4K", GT4HIP_VERBOSE="1"))
    assert code == 0 and out == "", err
    chunks = [ln for ln in err.split("\n") if " chunks" in ln]
    assert chunks and int(chunks[0].split(" of ")[1].split()[0]) >= 3, err
    assert left == {name: data}


@pytest.mark.gpu
def test_two_worker_processes_give_the_same_bytes(work):
    name, data = _expected_file(LARGEST)
    code, out, err, left = _run(_argv(LARGEST) + ["--gpus", "2"], work)
    assert (code, out, err) == (0, "", "")
    assert left == {name: data}
    code, out, err, left = _run(_argv(LARGEST), work, _env(GT4HIP_GPUS="2", GT4HIP_HBM_LIMIT="6K"))
    assert (code, out, err) == (0, "", "")
    assert left == {name: data}


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{}, {"GT4HIP_HBM_LIMIT": "4K"}], ids=["resident", "chunks"])
def test_count_only_prints_the_two_lines_of_the_union(env, work):
    for case in (LARGEST, next(c for c in CASES if c["inputs"] == "n2" and c["cutoff"] == 3 and c["min_lists"] == 1 and c["max_lists"] == 2)):
        code, out, err, left = _run(_argv(case) + ["--count_only"], work, _env(**env))
        assert (code, out, err, left) == (0, "NUnique\t%d\nNTotal\t%d\n" % (case["n_words"], case["total_count"]), "", {})


@pytest.mark.gpu
def test_debug_adds_nothing_and_either_option_is_enough(work):
    case = next(c for c in CASES if c["inputs"] == "n5" and c["rule"] == "default" and c["cutoff"] == 1 and (c["min_lists"], c["max_lists"]) == (5, 5))
    files = _files("n5")
    name, data = _expected_file(case)
    code, out, err, left = _run(files + ["-u", "--min_lists", "5", "-o", "s"], work)
    assert (code, out, err, left) == (0, "", "", {name: data})
    plain = _run(files + ["-u", "-o", "s", "-D"], work)
    code, out, err, left = _run(files + ["-u", "--min_lists", "5", "-o", "s", "-D"], work)
    assert (code, out, left) == (0, "", {name: data})
    assert err == "Rule: 0\nNum files: 5\n" and plain[2].startswith(err) and len(plain[2]) > len(err)
    case = next(c for c in CASES if c["inputs"] == "n5" and c["rule"] == "default" and c["cutoff"] == 1 and (c["min_lists"], c["max_lists"]) == (1, 1))
    name, data = _expected_file(case)
    assert _run(files + ["-u", "--max_lists", "1", "-o", "s"], work) == (0, "", "", {name: data})
