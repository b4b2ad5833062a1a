"""genometester4_amd/glistmaker against the reference's transcripts (tests/golden/gmaker_cases.json): every recorded
case replayed byte for byte, chunked runs against the unchunked one, and the result read by the drop-in glistquery."""
import os
import shutil
import subprocess

import pytest

import gmaker_util as U
import maker_model as M
from genometester4_amd.listio import parse_header

CASES = U.load_cases()
BY_ID = {c["id"]: c for c in CASES["cases"]}
READER_ERRORS = ("bad_start_k4", "no_plus_k4")


@pytest.fixture(scope="module")
def workdir():
    d = U.make_workdir(CASES)
    yield d
    shutil.rmtree(d, ignore_errors=True)


def _run(argv, cwd, env=None, stdin=None):
    return subprocess.run([U.BINARY] + argv, cwd=cwd, capture_output=True, env=dict(os.environ, **(env or {})), timeout=300, input=stdin)


def _check_list(case, data):
    if "list_hex" in case:
        assert data.hex() == case["list_hex"], case["id"]
    else:
        assert (len(data), U.sha(data)) == (case["list_bytes"], case["list_sha256"]), case["id"]


NO_DEVICE = [c for c in CASES["cases"] if c["id"].startswith(("err_", "version", "help"))]


@pytest.mark.parametrize("case", NO_DEVICE, ids=lambda c: c["id"])
def test_argv_errors_version_and_help_need_no_device(case, workdir):
    assert len(NO_DEVICE) >= 25
    p = _run(case["argv"], workdir, env=dict(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1"))
    assert (p.returncode, p.stdout.decode("latin-1"), p.stderr.decode("latin-1")) == (case["exit"], case["stdout"], case["stderr"])


def test_refused_forms_are_loud(workdir):
    hide = dict(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    p = _run(["multi.fa", "-w", "16", "--index", "-o", "idx"], workdir, env=hide)
    assert p.returncode == 1 and b"--index" in p.stderr
    with open(os.path.join(workdir, "z.fa.gz"), "wb") as f:
        f.write(b"\x1f\x8b\x08\x00rest")
    p = _run(["z.fa.gz", "-w", "16", "-o", "gz"], workdir, env=hide)
    assert p.returncode == 1 and b"gzip" in p.stderr
    p = _run(["multi.fa", "-w", "16", "-o", "nogpu"], workdir, env=hide)
    assert p.returncode == 1 and b"GPU" in p.stderr
    for name in ("idx_16.index", "idx_16.list", "gz_16.list", "nogpu_16.list", "nogpu_16.list.tmp"):
        assert not os.path.exists(os.path.join(workdir, name))


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in CASES["cases"] if c not in NO_DEVICE], ids=lambda c: c["id"])
def test_every_golden_replays_on_the_gpu(case, workdir):
    out = case["output"] or ("bad_4.list" if case["id"] in READER_ERRORS else None)
    if out and os.path.exists(os.path.join(workdir, out)):
        os.remove(os.path.join(workdir, out))
    p = _run(case["argv"], workdir)
    err = p.stderr.decode("latin-1")
    if case["id"] in READER_ERRORS:  # the reference's message for the first offending byte, then exit 1 and no list
        assert p.returncode == 1 and err.startswith(case["stderr"]) and "Error:" in err
        assert not os.path.exists(os.path.join(workdir, out)) and not os.path.exists(os.path.join(workdir, out + ".tmp"))
        return
    assert (p.returncode, p.stdout.decode("latin-1"), err) == (case["exit"], case["stdout"], case["stderr"])
    _check_list(case, open(os.path.join(workdir, case["output"]), "rb").read())
    assert not os.path.exists(os.path.join(workdir, case["output"] + ".tmp"))


# _pieces restates the cut rule of file_to_lists () in genometester4_amd/csrc/gt4_glistmaker_cli.c (len = chunk, then behind
# the memrchr '\n' of [len / 2, len)), and the replay reads that function's GT4HIP_VERBOSE lines "<id>: piece N ends at byte P"
# and "<id>: B bytes in N piece(s)": keep the three in step.
def _pieces(text, chunk):
    """where the program ends its pieces: `chunk` bytes, or behind the last '\\n' of the chunk's second half"""
    pos, ends = 0, []
    while pos < len(text):
        n = len(text) - pos
        if n > chunk:
            n = chunk
            nl = text.rfind(b"\n", pos + n // 2, pos + n)
            if nl >= 0:
                n = nl - pos + 1
        pos += n
        if pos < len(text):
            ends.append(pos)
    return ends


def _cut_kinds(text, k, ends):
    """which of the awkward places the cuts hit: inside a name, inside a quality line, k - 1 bases before a line end"""
    fastq, lines, start = text[:1] == b"@", [], 0
    while start < len(text):
        end = text.find(b"\n", start)
        end = len(text) if end < 0 else end
        role = ("name", "sequence", "plus", "quality")[len(lines) % 4] if fastq else ("name" if text[start:start + 1] == b">" else "sequence")
        lines.append((start, end, role))
        start = end + 1
    kinds = set()
    for p in ends:
        first, end, role = lines[_line_of(lines, p)]
        if p > first and role in ("name", "quality"):
            kinds.add(role)
        if p > first and role == "sequence" and end - p == k - 1:
            kinds.add("k-1")
    return kinds


def _line_of(lines, p):
    lo, hi = 0, len(lines) - 1
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if lines[mid][0] <= p else (lo, mid - 1)
    return lo


def _derived_chunk(text, k, want):
    """the largest chunk below two lines' length whose cuts hit every place in `want`"""
    for chunk in range(123, 4, -1):
        if want <= _cut_kinds(text, k, _pieces(text, chunk)):
            return chunk
    raise AssertionError("no chunk size cuts %s at %s" % (len(text), sorted(want)))


# the text above 100,000 bytes and the FastQ case at 4K and at a size derived from the fixture, so that the cuts are known
# to fall inside a name, inside a quality line and k - 1 bases before a line end (a FastA text has no quality line, and
# big.fa's three names are too few for a cut to meet one with fewer than 3000 pieces: multi.fa shows the FastA name)
CHUNKED = [("big_k25", "4K", None), ("big_k32", "4097", None), ("reads_fq_k16", "4K", None), ("big_k25", None, {"k-1"}),
           ("reads_fq_k16", None, {"name", "quality", "k-1"}), ("reads_fq_k5", "7", None), ("multi_fa_k16", None, {"name", "k-1"}), ("three_files_k25", "50", None)]


@pytest.mark.gpu
@pytest.mark.parametrize("cid,chunk,want", CHUNKED, ids=["%s-%s" % (c[0], c[1] or "derived") for c in CHUNKED])
def test_chunked_runs_write_the_same_list(cid, chunk, want, workdir):
    case = BY_ID[cid]
    k = int(case["argv"][case["argv"].index("-w") + 1])
    argv = [a if a != case["argv"][case["argv"].index("-o") + 1] else "chunked" for a in case["argv"]]
    texts = [U.file_bytes(CASES, a) for a in argv if a in CASES["files"]]
    if want:
        chunk = str(_derived_chunk(texts[0], k, want))
    chunk_bytes = int(chunk[:-1]) * 1024 if chunk.endswith("K") else int(chunk)
    out = os.path.join(workdir, "chunked_" + case["output"].split("_")[-1])
    p = _run(argv, workdir, env=dict(GT4HIP_MAKER_CHUNK=chunk, GT4HIP_VERBOSE="1"))
    assert p.returncode == 0, p.stderr
    err = p.stderr.decode().split("\n")
    names = [a for a in argv if a in CASES["files"]]
    for name, text in zip(names, texts):  # every text went through in the pieces expected: the cuts are where `want` was derived
        ends = [int(l.rsplit(" ", 1)[1]) for l in err if l.startswith(name + " block 0: piece ")]
        assert ends == _pieces(text, chunk_bytes), (name, chunk)
        assert ("%s block 0: %d bytes in %d piece(s)" % (name, len(text), len(ends) + 1)) in p.stderr.decode()
        assert len(ends) > 0 or len(text) <= chunk_bytes
    if want:
        assert want <= _cut_kinds(texts[0], k, _pieces(texts[0], chunk_bytes))
    _check_list(case, open(out, "rb").read())


@pytest.mark.gpu
def test_standard_input(workdir):
    case = BY_ID["multi_fa_k16"]
    p = _run(["-", "-w", "16", "-o", "stdin"], workdir, stdin=U.file_bytes(CASES, "multi.fa"))
    assert p.returncode == 0, p.stderr
    _check_list(case, open(os.path.join(workdir, "stdin_16.list"), "rb").read())


@pytest.mark.gpu
def test_glistquery_reads_the_result(workdir):
    case = BY_ID["big_k25"]
    p = _run(["big.fa", "-w", "25", "-o", "forquery"], workdir)
    assert p.returncode == 0, p.stderr
    data = M.list_bytes([U.file_bytes(CASES, "big.fa")], 25)
    assert U.sha(data) == case["list_sha256"]
    h = parse_header(data)
    q = subprocess.run([os.path.join(U.ROOT, "genometester4_amd", "glistquery"), "forquery_25.list", "--stat"], cwd=workdir, capture_output=True, timeout=300)
    assert q.returncode == 0
    assert q.stdout.decode() == "List forquery_25.list: built with glistmaker version 4.2\nWordlength\t25\nNUnique\t%d\nNTotal\t%d\n" % (h["n_words"], h["total_count"])
