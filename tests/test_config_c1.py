"""BASELINE.json configs[0] / SURVEY 8d C1: `glistcompare --intersection` on two 10 M-entry synthetic
k=16 .list files through the reference's own CPU path -- plumbing, no GPU: the reference binary and
the C restatement must agree on NUnique / NTotal and on every byte of the output file at this size
too.  What the reference printed and wrote for these lists is in tests/golden/c1_golden.json
(tests/golden/make_golden_c1.py); where oracle/_ref is built (oracle/Makefile), the binary is run
again as well.  With a GPU, the drop-in CLI is held to the same file."""
import hashlib
import json
import os
import subprocess
import tempfile

import pytest

import golden_util as GU
import oracle_lib as O
from genometester4_amd.listio import header_bytes, write_list

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "genometester4_amd", "glistcompare")
N, K = 10_000_000, 16
with open(os.path.join(ROOT, "tests", "golden", "c1_golden.json")) as _f:
    GOLDEN = json.load(_f)


def _sha(data):
    return hashlib.sha256(data).hexdigest()


@pytest.fixture(scope="module")
def c1():
    # shared universe: 1.5e7 ascending unique keys < 4^16; every third key is in both
    # lists, the others alternate between A and B: |A| = |B| = 1e7, |A n B| = 5e6
    a, b = GU.c1_lists(N)
    d = tempfile.mkdtemp(prefix="gt4c1_")
    write_list(os.path.join(d, "a.list"), a, K)
    write_list(os.path.join(d, "b.list"), b, K)
    exp = O.compare(a, b, O.OP_INTRSEC)[O.OP_INTRSEC]
    yield d, exp
    import shutil
    shutil.rmtree(d, ignore_errors=True)


def _run(exe, d, args):
    return subprocess.run([exe, "a.list", "b.list"] + args, cwd=d, capture_output=True, timeout=600)


def test_c1_reference_cpu_path_matches_restatement(c1):
    d, (n, total, rec) = c1
    assert n == N // 2
    for name in ("a.list", "b.list"):  # the very inputs the reference was given
        with open(os.path.join(d, name), "rb") as f:
            assert _sha(f.read()) == GOLDEN["inputs_sha256"][name], name
    assert GOLDEN["count_only_stdout"] == "NUnique\t%d\nNTotal\t%d\n" % (n, total)
    g = GOLDEN["intrsec"]
    assert (g["n_words"], g["total_count"]) == (n, total)
    assert _sha(header_bytes(K, n, total) + rec.tobytes()) == g["sha256"]
    if not os.access(O.REF_GLISTCOMPARE, os.X_OK):
        return  # (the reference binary itself, where oracle/_ref is built)
    r = _run(O.REF_GLISTCOMPARE, d, ["--intersection", "--count_only"])
    assert r.returncode == 0 and r.stdout.decode() == "NUnique\t%d\nNTotal\t%d\n" % (n, total)
    r = _run(O.REF_GLISTCOMPARE, d, ["--intersection", "-o", "ref"])
    assert r.returncode == 0
    with open(os.path.join(d, "ref_%d_intrsec.list" % K), "rb") as f:
        assert f.read() == header_bytes(K, n, total) + rec.tobytes()


@pytest.mark.gpu
def test_c1_drop_in_cli_writes_the_same_file(c1):
    d, (n, total, rec) = c1
    r = _run(CLI, d, ["--intersection", "-o", "hip"])
    assert r.returncode == 0, r.stderr.decode()
    with open(os.path.join(d, "hip_%d_intrsec.list" % K), "rb") as f:
        assert f.read() == header_bytes(K, n, total) + rec.tobytes()
