"""glistcompare --subset METHOD SIZE [--seed N] against the reference's transcripts (tests/golden/subset_cases.json):
exit code, stdout, stderr and the output file, byte for byte; what the reference does not survive (a walk that falls
short of SIZE) as an error; --gpus 2 refused; and without --seed the two properties that hold for every seed."""
import base64
import json
import os
import shutil
import sys
import tempfile

import numpy as np
import pytest

import subset_model as SM
from genometester4_amd.listio import read_list, write_list

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "genometester4_amd", "glistcompare")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_subset as MG  # noqa: E402

with open(os.path.join(ROOT, "tests", "golden", "subset_cases.json")) as _f:
    GOLDEN = json.load(_f)
RUNS = [c for c in GOLDEN["cases"] if c["exit"] == 0]
ERRORS = [c for c in GOLDEN["cases"] if c["exit"] != 0]
TIMEOUT = 60


@pytest.fixture(scope="module")
def work():
    d = tempfile.mkdtemp(prefix="gt4ss_cli_")
    files = MG.build_inputs(list(MG.INPUTS), d)
    for name, fn in files.items():
        assert MG.sha(os.path.join(d, fn)) == GOLDEN["inputs"][name]["sha256"], name
    # the shortfall inputs: 50 records with counts 1 .. 5
    write_list(os.path.join(d, "short50.list"), SM.make_list(50, 50, 13, 5), 13)
    files["short50"] = "short50.list"
    yield d, files
    shutil.rmtree(d, ignore_errors=True)


def _env():
    return {k: v for k, v in os.environ.items() if not k.startswith("GT4HIP_")}


def _replay(case, work):
    d, files = work
    code, out, err, left = MG.run_case(CLI, files, case["inputs"], case["argv"], os.path.join(d, "run_" + case["id"]), timeout=TIMEOUT, env=_env())
    want = {n: base64.b64decode(b) for n, b in case["files"].items()}
    assert (code, out, err) == (case["exit"], case["stdout"], case["stderr"]), case["id"]
    assert sorted(left) == sorted(want), case["id"]
    for n in want:
        assert left[n] == want[n], (case["id"], n)


@pytest.mark.gpu
@pytest.mark.parametrize("case", RUNS, ids=[c["id"] for c in RUNS])
def test_golden_replays_byte_for_byte(case, work):
    _replay(case, work)


@pytest.mark.parametrize("case", ERRORS, ids=[c["id"] for c in ERRORS])
def test_error_transcripts_need_no_device(case, work):
    assert len(ERRORS) >= 5
    _replay(case, work)


def test_several_gpus_and_a_memory_limit_are_refused(work):
    d, files = work
    code, out, err, left = MG.run_case(CLI, files, ["c300"], ["--subset", "rand", "10", "--seed", "1", "--gpus", "2"], os.path.join(d, "run_gpus"), env=_env())
    assert (code, out, left) == (1, "", {}) and "--subset needs the list resident on one GPU" in err and "--gpus" in err
    code, out, err, left = MG.run_case(CLI, files, ["c300"], ["--subset", "rand", "10", "--seed", "1"], os.path.join(d, "run_hbm"),
                                       env=dict(_env(), GT4HIP_HBM_LIMIT="1G"))
    assert (code, out, left) == (1, "", {}) and "GT4HIP_HBM_LIMIT" in err
    # the reference's own checks come first
    code, out, err, left = MG.run_case(CLI, files, ["c300"], ["--subset", "rand_unique", "301", "--gpus", "2"], os.path.join(d, "run_gpus2"), env=_env())
    assert code == 1 and err == "Error: Unique subset size (301) is bigger than number of unique kmers (300)\n"


@pytest.mark.gpu
@pytest.mark.parametrize("method,size", [("rand_weighted_unique", 45), ("rand", None)])
def test_a_walk_that_falls_short_is_an_error_and_leaves_no_file(method, size, work):
    """the reference does not terminate on these (n = 50, counts 1 .. 5, rand_weighted_unique 45: still running after
    60 s; rand with SIZE = sum_counts + 1 walks past the list)"""
    d, files = work
    rec = SM.make_list(50, 50, 13, 5)
    if size is None:
        size = int(rec["count"].sum()) + 1
    with pytest.raises(SM.Shortfall) as short:
        SM.serial_walk(rec, {"rand": SM.RAND, "rand_weighted_unique": SM.RAND_WEIGHTED_UNIQUE}[method], size, SM.state48(5))
    code, out, err, left = MG.run_case(CLI, files, ["short50"], ["--subset", method, str(size), "--seed", "5"], os.path.join(d, "run_short_" + method),
                                       timeout=TIMEOUT, env=_env())
    print(err)
    assert (code, out, left) == (1, "", {})
    assert err.startswith("Error: ") and err.count("\n") == 1
    assert "%s %d" % (method, size) in err and "only %d of %d" % (short.value.reached, size) in err


@pytest.mark.gpu
def test_without_a_seed_the_size_is_met(work):
    d, files = work
    rec, _ = MG.input_records("c300")
    code, out, err, left = MG.run_case(CLI, files, ["c300"], ["--subset", "rand_unique", "77"], os.path.join(d, "run_noseed_u"), timeout=TIMEOUT, env=_env())
    assert (code, out, err, sorted(left)) == (0, "", "", ["out_subset_13.list"])
    with open(os.path.join(d, "noseed_u.list"), "wb") as f:
        f.write(left["out_subset_13.list"])
    h, got = read_list(os.path.join(d, "noseed_u.list"))
    assert h["n_words"] == len(got) == 77 and h["total_count"] == int(got["count"].sum())
    at = np.searchsorted(rec["key"], got["key"])
    assert np.all(got["key"][1:] > got["key"][:-1]) and rec[at].tobytes() == got.tobytes()
    code, out, err, left = MG.run_case(CLI, files, ["c300"], ["--subset", "rand", "1234"], os.path.join(d, "run_noseed_r"), timeout=TIMEOUT, env=_env())
    assert (code, out, err, sorted(left)) == (0, "", "", ["out_subset_13.list"])
    with open(os.path.join(d, "noseed_r.list"), "wb") as f:
        f.write(left["out_subset_13.list"])
    h, got = read_list(os.path.join(d, "noseed_r.list"))
    assert h["total_count"] == int(got["count"].sum()) == 1234 and h["n_words"] == len(got)
    at = np.searchsorted(rec["key"], got["key"])
    assert np.array_equal(rec["key"][at], got["key"]) and np.all(got["count"] <= rec["count"][at]) and np.all(got["count"] > 0)


def test_a_build_without_the_entry_point_says_so(work):
    """tests/harness links the command line against a CPU stand-in that has no gt4hip_list_subset: the weak symbol is
    absent, and --subset is an error after the reference's own checks"""
    import subprocess
    harness = os.path.join(ROOT, "tests", "harness")
    r = subprocess.run(["make", "-C", harness, "_build/glistcompare_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    d, files = work
    stub = os.path.join(harness, "_build", "glistcompare_asan")
    code, out, err, left = MG.run_case(stub, files, ["c300"], ["--subset", "rand", "10", "--seed", "7"], os.path.join(d, "run_stub"), env=_env())
    assert (code, out, err, left) == (1, "", "Error: this build has no --subset path\n", {})
    code, out, err, left = MG.run_case(stub, files, ["c300"], ["--subset", "rand_unique", "301", "--seed", "7"], os.path.join(d, "run_stub2"), env=_env())
    assert (code, err) == (1, "Error: Unique subset size (301) is bigger than number of unique kmers (300)\n")
