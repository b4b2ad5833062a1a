"""genometester4_amd/glistquery --per_sequence against tests/golden/gqseq_cases.json (made by
tests/golden/make_golden_gqseq.py from oracle/_ref/glistquery alone).

Without a GPU: what argv alone refuses is refused with one "Error:" line, exit 1 and an empty stdout, no device opened.
With one (pytest.mark.gpu): every case byte for byte, and again with GT4HIP_QUERY_CHUNK = 1, 7 and 64 bytes, where
sequences, names and words span the pieces the file goes through the device in."""
import os
import shutil
import subprocess

import pytest

import gqseq_util as U

CASES = U.CASES["cases"]
REFUSED = [c for c in CASES if c["kind"] == "argv"]


@pytest.fixture(scope="module")
def workdir():
    d = U.make_workdir()
    yield d
    shutil.rmtree(d, ignore_errors=True)


def _run(argv, cwd, chunk=None, hide_gpu=False):
    env = {k: v for k, v in os.environ.items() if k != "GT4HIP_QUERY_CHUNK"}
    if chunk is not None:
        env["GT4HIP_QUERY_CHUNK"] = str(chunk)
    if hide_gpu:
        env.update(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    return subprocess.run([U.BINARY] + argv, cwd=cwd, capture_output=True, env=env, timeout=300)


@pytest.mark.parametrize("case", REFUSED, ids=lambda c: c["id"])
def test_refused_by_argv_alone_without_a_device(case, workdir):
    p = _run(case["argv"], workdir, hide_gpu=True)
    err = p.stderr.decode("latin-1")
    assert p.returncode == 1 and p.stdout == b"", (p.returncode, p.stdout, err)
    assert err.startswith("Error: ") and err.count("\n") == 1 and "GPU" not in err, err


def test_a_profile_without_a_device_fails_loudly(workdir):
    from genometester4_amd import capi
    p = _run(["K9.list", "-s", "small.fa", "--per_sequence"], workdir)
    if capi.lib().gt4hip_device_count() > 0:
        assert p.returncode == 0 and p.stdout, p.stderr
    else:  # no CPU path
        assert p.returncode == 1 and p.stdout == b"" and b"GPU" in p.stderr, p.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_every_golden_replays_on_the_gpu(case, workdir):
    p = _run(case["argv"], workdir)
    assert p.returncode == case["exit"], p.stderr.decode("latin-1")
    assert p.stdout.decode("latin-1") == case["stdout"]


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [1, 7, 64])
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_every_golden_replays_in_small_pieces(case, chunk, workdir):
    p = _run(case["argv"], workdir, chunk=chunk)
    assert p.returncode == case["exit"], p.stderr.decode("latin-1")
    assert p.stdout.decode("latin-1") == case["stdout"]


@pytest.mark.gpu
def test_verbose_names_the_pieces_and_the_kernel_times(workdir):
    env = dict(os.environ, GT4HIP_VERBOSE="1", GT4HIP_QUERY_CHUNK="64")
    p = subprocess.run([U.BINARY, "K9.list", "-s", "small.fa", "--per_sequence"], cwd=workdir, capture_output=True, env=env, timeout=300)
    err = p.stderr.decode("latin-1")
    assert p.returncode == 0 and "piece 2 ends at byte" in err and "lookups and sums" in err and "piece(s)" in err, err
    assert p.stdout.decode("latin-1") == [c for c in CASES if c["id"] == "k9_fa"][0]["stdout"]
