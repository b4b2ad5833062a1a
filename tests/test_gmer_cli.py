"""genometester4_amd/gmer_counter against the reference's transcripts (tests/golden/gmer_cases.json): the cases that
need no device with the devices hidden, the forms the drop-in refuses, every other case byte for byte on the GPU, and
chunked runs against the unchunked transcript."""
import os
import shutil
import subprocess

import pytest

import gmer_model as M
import gmer_util as U

CASES = U.load_cases()
BY_ID = {c["id"]: c for c in CASES["cases"]}
HIDE = dict(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
PAD = b"# " + b"x" * 300 + b"\n"


@pytest.fixture(scope="module")
def workdir():
    d = U.make_workdir(CASES)
    yield d
    shutil.rmtree(d, ignore_errors=True)


def _run(argv, cwd, env=None):
    return subprocess.run([U.BINARY] + argv, cwd=cwd, capture_output=True, env=dict(os.environ, **(env or {})), timeout=300)


def _check(case, p):
    err = p.stderr.decode("latin-1")
    if case["first_stderr_line_only"]:
        err = err.split("\n")[0] + "\n"
    assert (p.returncode, err) == (case["exit"], case["stderr"]), case["id"]
    assert U.stdout_matches(case, p.stdout), (case["id"], p.stdout[:400])


NO_DEVICE = [c for c in CASES["cases"] if not c["device"]]


@pytest.mark.parametrize("case", NO_DEVICE, ids=lambda c: c["id"])
def test_argv_and_database_errors_version_and_help_need_no_device(case, workdir):
    assert len(NO_DEVICE) == 21
    _check(case, _run(case["argv"], workdir, env=HIDE))


REFUSED_DBS = {
    "dup_rc.txt": (PAD + b"n1\t2\tACGTA\tTACGT\n", b"k-mers 0 and 1"),
    "dup_nodes.txt": (PAD + b"n1\t1\tACGTA\nn2\t2\tCCCCC\tACGTA\n", b"k-mers 0 and 2"),
    "short_node.txt": (PAD + b"n1\t3\tACGTA\tCCCCC\nn2\t1\tGGGTT\n", b"fewer than it declares"),
    "short_kmer.txt": (PAD + b"n1\t1\tACGTA\nn2\t1\tACG\n", b"shorter than the word length"),
    "no_base.txt": (PAD + b"n1\t1\tACGTA\nn2\t1\tACNTA\n", b"no base"),
    "no_newline.txt": (PAD + b"n1\t1\tACGTA", b"newline"),
    "no_wordlength.txt": (PAD + b"n1\t0\nn2\t1\tACGTA\n", b"word length"),
    "long_kmer.txt": (PAD + b"n1\t1\t" + b"A" * 33 + b"\n", b"at most 32"),
}


def test_refused_forms_are_loud_and_leave_nothing_behind(workdir):
    before = sorted(os.listdir(workdir))

    def refused(argv, *needles):
        p = _run(argv, workdir, env=HIDE)
        lines = p.stderr.decode("latin-1").split("\n")
        assert p.returncode == 1 and p.stdout == b"" and lines[0].startswith("Error: ") and lines[1:] == [""], (argv, p.stderr)
        for n in needles:
            assert n in p.stderr, (argv, p.stderr)

    for opt in ("-dbb", "-w", "--compile_index"):
        refused([opt, "x.bin", "multi.fa"], opt.encode())
        refused(["-db", "db25.txt", "multi.fa", opt, "x.bin"] if opt != "-dbb" else [opt, "x.bin", "multi.fa", "--stats"], opt.encode())
    for opt in ("--export_reads", "--dump_index", "--count_trie_allocations"):
        refused(["-db", "db25.txt", opt, "multi.fa"], opt.encode())
    refused(["multi.fa"], b"-db")
    refused(["-db", "db25.txt", "-"], b"standard input")
    refused(["-db", "db25.txt", "multi.fa", "-"], b"standard input")
    with open(os.path.join(workdir, "z.fa.gz"), "wb") as f:
        f.write(b"\x1f\x8b\x08\x00rest")
    refused(["-db", "db25.txt", "z.fa.gz"], b"gzip")
    os.remove(os.path.join(workdir, "z.fa.gz"))
    for name, (text, needle) in REFUSED_DBS.items():
        with open(os.path.join(workdir, name), "wb") as f:
            f.write(text)
        with pytest.raises(M.Refused):
            M.parse_db(text)
        refused(["-db", name, "multi.fa"], needle, name.encode())
        os.remove(os.path.join(workdir, name))
    with open(os.path.join(workdir, "odd.txt"), "wb") as f:
        f.write(PAD + b"n1\t2\tACGTA\tCCCCC\nn2\t1\tGGGTT\n")
    refused(["-db", "odd.txt", "--double_median", "multi.fa"], b"--double_median")
    os.remove(os.path.join(workdir, "odd.txt"))
    # a well-formed run without a device fails loudly too: there is no CPU path
    p = _run(["-db", "db25.txt", "multi.fa"], workdir, env=HIDE)
    assert p.returncode == 1 and p.stdout == b"" and b"GPU" in p.stderr
    assert sorted(os.listdir(workdir)) == before


ON_DEVICE = [c for c in CASES["cases"] if c["device"]]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ON_DEVICE, ids=lambda c: c["id"])
def test_every_golden_replays_on_the_gpu(case, workdir):
    assert len(ON_DEVICE) == 55
    _check(case, _run(case["argv"], workdir))


@pytest.mark.gpu
def test_recover_is_accepted_and_not_honoured(workdir):
    case = BY_ID["err_bad_start"]
    p = _run(case["argv"] + ["--recover"], workdir)
    err = p.stderr.decode("latin-1")
    assert p.returncode == 1 and p.stdout == b"" and err.startswith(case["stderr"])
    rest = err[len(case["stderr"]):].split("\n")
    assert len(rest) == 2 and rest[0].startswith("Error: ") and "--recover" in rest[0] and rest[1] == ""


CHUNKED = [(cid, chunk) for cid in ("big_stats_all", "three_files", "big_k25_small_db", "fastq_stats_k16") for chunk in ("4096", "65536", "1237")] + \
          [("three_files_k5", "7"), ("polya_32", "4K")]


@pytest.mark.gpu
@pytest.mark.parametrize("cid,chunk", CHUNKED, ids=["%s-%s" % c for c in CHUNKED])
def test_chunked_runs_print_the_same(cid, chunk, workdir):
    case = BY_ID[cid]
    p = _run(case["argv"], workdir, env=dict(GT4HIP_GMER_CHUNK=chunk, GT4HIP_VERBOSE="1"))
    assert p.returncode == case["exit"] == 0, p.stderr
    assert U.stdout_matches(case, p.stdout), p.stdout[:400]
    chunk_bytes = int(chunk[:-1]) * 1024 if chunk.endswith("K") else int(chunk)
    err = p.stderr.decode("latin-1")
    for name in (a for a in case["argv"] if a in CASES["files"] and not a.startswith("db")):  # every text went through in pieces of at most the chunk
        size = len(U.file_bytes(CASES, name))
        line = next(l for l in err.split("\n") if l.startswith("%s: %d bytes in " % (name, size)))
        pieces = int(line.split(" bytes in ")[1].split(" ")[0])
        assert pieces >= -(-size // chunk_bytes) and (pieces > 1 or size <= chunk_bytes), line
