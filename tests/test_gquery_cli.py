"""genometester4_amd/glistquery against the reference's transcripts (tests/golden/gquery_cases.json, made by
tests/golden/make_golden_gquery.py from oracle/_ref/glistquery).

Without a GPU: the early errors, --stat, -v, -h and the dump of one list open no device and must already print the
reference's bytes; the -f and FastA / FastQ parsers are reached through --words-only and held to tests/query_model.py.
With one (pytest.mark.gpu): EVERY recorded case, stdout and exit code byte for byte, and the multi-list forms of
tests/golden/query_cases.json through the reference's own argv."""
import json
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import golden_util as G
import gquery_util as U
import query_model as M
from genometester4_amd.listio import RECORD_DTYPE, write_list

CASES = U.CASES["cases"]
# what the header comment of gt4_glistquery_cli.c promises to work with no device
NO_DEVICE = [c for c in CASES if c["id"].startswith(("err_", "stat_", "dump_", "version", "help", "warn_no_query")) or c["id"].endswith("_err") and "_p" in c["id"]]


@pytest.fixture(scope="module")
def workdir():
    d = U.make_workdir()
    yield d
    shutil.rmtree(d, ignore_errors=True)


def _run(argv, cwd, hide_gpu=False):
    env = dict(os.environ)
    if hide_gpu:
        env.update(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    return subprocess.run([U.BINARY] + argv, cwd=cwd, capture_output=True, env=env, timeout=300)


@pytest.mark.parametrize("case", NO_DEVICE, ids=lambda c: c["id"])
def test_no_device_cases_replay(case, workdir):
    assert len(NO_DEVICE) >= 30
    p = _run(case["argv"], workdir, hide_gpu=True)
    assert p.returncode == case["exit"], p.stderr.decode("latin-1")
    U.check_stdout(case, p.stdout)
    if "stderr" in case and case["id"] not in ("err_wordlength", "err_missing_list"):
        assert p.stderr.decode("latin-1") == case["stderr"]


def test_a_lookup_without_a_device_fails_loudly(workdir):
    from genometester4_amd import capi
    have = capi.lib().gt4hip_device_count() > 0
    for argv in (["L16.list", "-q", "CCAGAAAATAGCGACG", "-mm", "1"], ["A8.list", "--median"], ["A8.list", "--gc"], ["A8.list", "--distribution", "3"]):
        p = _run(argv, workdir)
        if have:
            assert p.returncode == 0 and p.stdout, (argv, p.stderr)
        else:  # no CPU path
            assert p.returncode == 1 and p.stdout == b"" and b"GPU" in p.stderr, (argv, p.stderr)


def test_refused_options_are_loud(workdir):
    for opt in ("--locations", "--files", "--sequences"):
        p = _run(["A8.list", opt], workdir, hide_gpu=True)
        assert p.returncode == 1 and p.stdout == b"" and opt.encode() in p.stderr
    p = _run(["A8.list", "-s", "nothere.fa", "--words-only"], workdir, hide_gpu=True)  # (the reference: a failed assertion, exit 255)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr == b"search_fasta: Cannot open nothere.fa\n"
    with open(os.path.join(workdir, "z.fa.gz"), "wb") as f:
        f.write(b"\x1f\x8b\x08\x00rest")
    p = _run(["A8.list", "-s", "z.fa.gz", "--words-only"], workdir, hide_gpu=True)
    assert p.returncode == 1 and b"gzip" in p.stderr


@pytest.mark.parametrize("name", sorted(n for n in U.CASES["files"] if n.endswith((".fa", ".fq", ".txt"))))
def test_parsers_give_the_model_s_words(name, workdir):
    """--words-only prints the words before they are canonicalised and looked up; no device"""
    k = {"q4.txt": 4, "q32.txt": 32, "q12.txt": 12, "reads25.fa": 25, "s8.fa": 8}.get(name, 16)
    lst = {4: "K4", 32: "K32", 12: "R1", 25: "G25", 8: "A8", 16: "L16"}[k] + ".list"
    text = U.CASES["files"][name]
    for extra in ([], ["--3p"], ["--5p"]):
        if name.endswith(".txt"):
            words, rc = M.query_file_words(text, k, "--3p" in extra, "--5p" in extra)
            opt = "-f"
        else:
            words, rc = M.fasta_words(text, k)
            rc &= 0xFF
            opt = "-s"
        p = _run([lst, opt, name, "--words-only"] + extra, workdir, hide_gpu=True)
        assert p.returncode == rc, p.stderr
        assert [int(x) for x in p.stdout.split()] == words


def test_host_source_names_no_reference_file():
    for name in ("gt4_glistquery_cli.c", "gt4_cli.c"):
        src = open(os.path.join(U.ROOT, "genometester4_amd", "csrc", name)).read()
        assert "#include \"gt4hip.h\"" in src and "word-map.h" not in src, name


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_every_golden_replays_on_the_gpu(case, workdir):
    p = _run(case["argv"], workdir)
    assert p.returncode == case["exit"], p.stderr.decode("latin-1")
    U.check_stdout(case, p.stdout)


Q = json.load(open(os.path.join(U.ROOT, "tests", "golden", "query_cases.json")))


@pytest.fixture(scope="module")
def multi_workdir():
    _, inputs, _ = G.load()
    d = tempfile.mkdtemp(prefix="gt4gquery_multi_")
    for name in Q["inputs"]:
        rec, k, _ = inputs[name]
        write_list(os.path.join(d, name + ".list"), rec, k)
    for name, (hexbytes, k) in Q["extra_inputs"].items():
        write_list(os.path.join(d, name + ".list"), np.frombuffer(bytes.fromhex(hexbytes), dtype=RECORD_DTYPE), k)
    yield d
    shutil.rmtree(d, ignore_errors=True)


@pytest.mark.gpu
@pytest.mark.parametrize("case", Q["cases"], ids=lambda c: c["id"])
def test_multi_list_forms_through_the_reference_argv(case, multi_workdir):
    p = _run(case["ref_argv"], multi_workdir)
    assert p.returncode == case["exit"], p.stderr.decode("latin-1")
    assert p.stdout.decode("latin-1") == case["stdout"]
