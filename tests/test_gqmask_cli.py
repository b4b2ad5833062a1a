"""`glistquery LIST -s FILE --mask [--soft_mask]` through the binary: tests/golden/gqmask_cases.json (made by
tests/golden/make_golden_gqmask.py from the reference's glistquery) replayed.  Without a GPU: what argv alone refuses, in
front of any device.  With one (pytest.mark.gpu): every case byte for byte with its exit status, whole and with
GT4HIP_QUERY_CHUNK = 1, 7 and 64 bytes, where the hold-back of the output crosses many pieces; the malformed file with the
reader's line on stderr."""
import os
import shutil
import subprocess

import pytest

import gqmask_util as U

CASES = U.COMPUTED + U.MALFORMED


@pytest.fixture(scope="module")
def workdir():
    d = U.make_workdir()
    yield d
    shutil.rmtree(d, ignore_errors=True)


def _run(argv, cwd, chunk=None, hide_gpu=False, verbose=False):
    env = {k: v for k, v in os.environ.items() if k not in ("GT4HIP_QUERY_CHUNK", "GT4HIP_VERBOSE")}
    if chunk is not None:
        env["GT4HIP_QUERY_CHUNK"] = str(chunk)
    if verbose:
        env["GT4HIP_VERBOSE"] = "1"
    if hide_gpu:
        env.update(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    return subprocess.run([U.BINARY] + argv, cwd=cwd, capture_output=True, env=env, timeout=300)


@pytest.mark.parametrize("case", U.REFUSED, ids=lambda c: c["id"])
def test_refused_by_argv_alone_without_a_device(case, workdir):
    p = _run(case["argv"], workdir, hide_gpu=True)
    err = p.stderr.decode("latin-1")
    assert p.returncode == 1 and p.stdout == b"", (p.returncode, p.stdout, err)
    assert err.startswith("Error: ") and err.count("\n") == 1 and "GPU" not in err and "nknown" not in err, err


def test_masking_without_a_device_fails_loudly(workdir):
    from genometester4_amd import capi
    p = _run(["K9.list", "-s", "small.fa", "--mask"], workdir)
    if capi.lib().gt4hip_device_count() > 0:
        assert p.returncode == 0 and p.stdout, p.stderr
    else:  # no CPU path
        assert p.returncode == 1 and p.stdout == b"" and b"GPU" in p.stderr, p.stderr


def test_the_help_screen_is_still_the_reference_s(workdir):
    p = _run(["-h"], workdir, hide_gpu=True)
    assert p.returncode == 0 and b"mask" not in p.stderr + p.stdout


def _check(p, case):
    err = p.stderr.decode("latin-1")
    assert p.returncode == case["exit"] % 256, err
    assert p.stdout.decode("latin-1") == case["stdout"]
    if case["kind"] == "malformed":
        assert err.splitlines() == [case["stderr"]]
    else:
        assert err == ""


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_every_golden_replays_on_the_gpu(case, workdir):
    _check(_run(case["argv"], workdir), case)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [1, 7, 64])
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_every_golden_replays_in_small_pieces(case, chunk, workdir):
    _check(_run(case["argv"], workdir, chunk=chunk), case)


@pytest.mark.gpu
def test_a_nul_ends_the_masking_and_the_rest_is_copied(workdir):
    text = U.text_of("small.fa")
    at = len(text) // 2
    with open(os.path.join(workdir, "nul.fa"), "wb") as f:
        f.write(text[:at] + b"\0" + text[at + 1:])
    import mask_model as MM
    keys, counts, k = U.keys_counts("ALL9")
    want = MM.mask_text(keys, counts, text[:at] + b"\0" + text[at + 1:], k).text
    assert want[at:] == b"\0" + text[at + 1:] and want[:at] != text[:at]
    for chunk in (None, 7, 64):
        p = _run(["ALL9.list", "-s", "nul.fa", "--mask"], workdir, chunk=chunk)
        assert p.returncode == 0 and p.stdout == want, (chunk, p.stderr)


@pytest.mark.gpu
def test_verbose_names_the_pieces(workdir):
    p = _run(["K9.list", "-s", "small.fa", "--mask"], workdir, chunk=64, verbose=True)
    err = p.stderr.decode("latin-1")
    assert p.returncode == 0 and "pieces of 64 bytes" in err and "lookups and masking" in err and "piece(s)" in err, err
