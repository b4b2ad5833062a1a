"""`glistmaker --index` against the reference's own index files (tests/golden/gindex_cases.json): every recorded case
replayed, the same in small pieces, and the result read by the drop-in glistcompare and by the reference's glistquery.
The four bytes of the file block that the reference leaves undefined (tests/index_model.MASKED) are masked on both sides."""
import glob
import hashlib
import os
import shutil
import subprocess
import tempfile

import pytest

import gindex_util as G
import gmaker_util as U
import index_model as IM
from genometester4_amd.listio import parse_header

GOLDEN, GOLDEN_FILES = G.load()
BY_ID = {c["id"]: c for c in GOLDEN["cases"]}
COMPARE = os.path.join(U.ROOT, "genometester4_amd", "glistcompare")
REF_QUERY = os.path.join(U.ROOT, "oracle", "_ref", "glistquery")
HIDE = dict(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")


@pytest.fixture(scope="module")
def workdir():
    d = tempfile.mkdtemp(prefix="gt4gindex_cli_")
    for name in GOLDEN["files"]:
        with open(os.path.join(d, name), "wb") as f:
            f.write(G.file_bytes(GOLDEN, name))
    yield d
    shutil.rmtree(d, ignore_errors=True)


def _run(argv, cwd, env=None, stdin=None):
    return subprocess.run([U.BINARY] + argv, cwd=cwd, capture_output=True, env=dict(os.environ, **(env or {})), timeout=300, input=stdin)


def _check_index(case, path):
    data = IM.masked(open(path, "rb").read())
    if case["id"] in GOLDEN_FILES:
        assert data == GOLDEN_FILES[case["id"]], case["id"]
    assert (len(data), hashlib.sha256(data).hexdigest()) == (case["bytes"], case["sha256"]), case["id"]
    assert not os.path.exists(path + ".tmp")


# ---- no device: what --index says before it needs one

ARGV_ERRORS = [
    (["--index"], "Error: No FastA/FastQ file specified!\n"),
    (["multi.fa", "--index", "-w", "0"], "Error: Invalid word-length 0 (must be 1 - 32)!\n"),
    (["multi.fa", "--index", "-w", "33"], "Error: Invalid word-length 33 (must be 1 - 32)!\n"),
    (["multi.fa", "--index", "-w", "16", "-c", "0"], "Error: Invalid frequency cut-off: 0! Must be positive.\n"),
    (["multi.fa", "--index", "-w", "16", "-c", "3", "--max", "2"], "Error: Invalid frequency range: 3-2!\n"),
    (["multi.fa", "--index", "-w", "x"], "Error: Invalid word-length: x! Must be an integer.\n"),
    (["absent.fa", "--index", "-w", "16"], "main: No such file (cannot stat): absent.fa\n"),
]


@pytest.mark.parametrize("argv,message", ARGV_ERRORS, ids=[" ".join(a[0]) for a in ARGV_ERRORS])
def test_argv_errors_of_index_forms_need_no_device(argv, message, workdir):
    """the messages of the reference's main() (src/glistmaker.c:158-264), which come before any file is read"""
    p = _run(argv + ["-o", "argv_err"], workdir, env=HIDE)
    assert p.returncode == 1 and p.stdout == b""
    assert p.stderr.decode("latin-1").startswith(message) or message in p.stderr.decode("latin-1")
    assert not glob.glob(os.path.join(workdir, "argv_err_*"))


def test_index_without_a_device_or_from_standard_input_is_refused(workdir):
    p = _run(["multi.fa", "-w", "16", "--index", "-o", "nodev"], workdir, env=HIDE)
    assert p.returncode == 1 and b"--index" in p.stderr and b"GPU" in p.stderr
    p = _run(["-", "-w", "16", "--index", "-o", "nodev"], workdir, env=HIDE, stdin=b">a\nACGT\n")
    assert p.returncode == 1 and b"--index" in p.stderr and b"standard input" in p.stderr
    assert not glob.glob(os.path.join(workdir, "nodev_*"))


def test_help_text_still_offers_index(workdir):
    p = _run(["-h"], workdir, env=HIDE)
    assert p.returncode == 0 and b"    --index                 - create index instead of list\n" in p.stderr


# ---- on the device

@pytest.mark.gpu
@pytest.mark.parametrize("case", GOLDEN["cases"], ids=[c["id"] for c in GOLDEN["cases"]])
def test_every_golden_index_replays_on_the_gpu(case, workdir):
    out = os.path.join(workdir, case["output"])
    if os.path.exists(out):
        os.remove(out)
    p = _run(case["argv"], workdir)
    assert p.returncode == case["exit"], p.stderr
    _check_index(case, out)


# pieces far smaller than a tile, a line or a name (every carry of the locations travels many times), and pieces around a
# tile for the texts above one; `-c` / `--max` and several files among them
CHUNKED = [("multi_k11", "7"), ("reads_k16", "7"), ("reads_k2", "50"), ("three_files_k11", "50"), ("lowc_c2_max3_k11", "64"), ("many_k5", "100"),
           ("long_name_k11", "1000"), ("long_k16", "4097"), ("pos256_k11", "33"), ("big_k25", "4K"), ("crlf_k11", "9"), ("nofinal_k11", "13")]


@pytest.mark.gpu
@pytest.mark.parametrize("cid,chunk", CHUNKED, ids=["%s-%s" % c for c in CHUNKED])
def test_chunked_runs_write_the_same_index(cid, chunk, workdir):
    case = BY_ID[cid]
    argv = [a if a != cid else "chunked_" + cid for a in case["argv"]]
    p = _run(argv, workdir, env=dict(GT4HIP_MAKER_CHUNK=chunk, GT4HIP_VERBOSE="1"))
    assert p.returncode == 0, p.stderr
    pieces = [l for l in p.stderr.decode().split("\n") if " block 0: piece " in l]
    assert len(pieces) >= 2, p.stderr
    _check_index(case, os.path.join(workdir, "chunked_" + case["output"]))


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["multi_k16", "big_k25"])
def test_glistcompare_finds_the_index_equal_to_the_list(cid, workdir):
    """x.index and the x.list of the same text hold the same words: no difference either way, everything in common"""
    case = BY_ID[cid]
    k = case["k"]
    assert _run(case["inputs"] + ["-w", str(k), "-o", "cmpidx", "--index"], workdir).returncode == 0
    assert _run(case["inputs"] + ["-w", str(k), "-o", "cmplst"], workdir).returncode == 0
    n_words = parse_header(open(os.path.join(workdir, "cmplst_%d.list" % k), "rb").read())["n_words"]
    assert n_words == IM.parse(open(os.path.join(workdir, "cmpidx_%d.index" % k), "rb").read())["n_kmers"] > 100
    p = subprocess.run([COMPARE, "cmpidx_%d.index" % k, "cmplst_%d.list" % k, "-d", "-dd", "-i", "-o", "cmp" + cid], cwd=workdir, capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr
    found = {}
    for kind in ("intrsec", "diff1", "diff2"):
        names = glob.glob(os.path.join(workdir, "cmp%s_%d_*%s.list" % (cid, k, kind)))  # (<out>_<k>_intrsec.list, <out>_<k>_0_diff1.list)
        assert len(names) == 1, (kind, names)
        found[kind] = parse_header(open(names[0], "rb").read())["n_words"]
    assert found == dict(intrsec=n_words, diff1=0, diff2=0)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["multi_k11", "two_files_k16", "lowc_c2_k11"])
def test_the_reference_glistquery_reads_our_index_like_its_own(cid, workdir):
    """`glistquery x.index --stat` of the reference on our file and on the reference's file; where the reference binaries
    are not built, what it prints for its own file is restated from that file's header"""
    case = BY_ID[cid]
    assert _run([a if a != cid else "stat_" + cid for a in case["argv"]], workdir).returncode == 0
    ours = "stat_" + case["output"]
    theirs = IM.parse(GOLDEN_FILES[cid])
    want = "Index %%s: built with glistmaker version 4.2\nWordlength\t%d\nNUnique\t%d\nNTotal\t%d\n" % (case["k"], theirs["n_kmers"], theirs["n_locations"])
    mine = IM.parse(open(os.path.join(workdir, ours), "rb").read())
    assert (mine["k"], mine["n_kmers"], mine["n_locations"]) == (case["k"], theirs["n_kmers"], theirs["n_locations"])
    if os.path.exists(REF_QUERY):
        with open(os.path.join(workdir, "ref_" + case["output"]), "wb") as f:
            f.write(GOLDEN_FILES[cid])
        for name in (ours, "ref_" + case["output"]):
            q = subprocess.run([REF_QUERY, name, "--stat"], cwd=workdir, capture_output=True, timeout=300)
            assert (q.returncode, q.stdout.decode()) == (0, want % name), q.stderr
