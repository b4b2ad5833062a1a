"""tests/gmer_model.py against the reference's own transcripts (tests/golden/gmer_cases.json): every golden is replayed
through the model byte for byte, which is what lets the GPU tests use the model on inputs that have no golden."""
import pytest

import gmer_model as M
import gmer_util as U

CASES = U.load_cases()
IDS = [c["id"] for c in CASES["cases"]]


def read_file(name):
    return U.file_bytes(CASES, name) if name in CASES["files"] else None


def test_the_goldens_are_all_there():
    assert len(IDS) == len(set(IDS)) == 76
    assert sum(1 for c in CASES["cases"] if not c["device"]) == 21
    assert sum(1 for c in CASES["cases"] if c["first_stderr_line_only"]) == 1


@pytest.mark.parametrize("cid", IDS)
def test_model_replays_golden(cid):
    case = next(c for c in CASES["cases"] if c["id"] == cid)
    code, out, err = M.run(case["argv"], read_file)
    if case["first_stderr_line_only"]:
        err = err.split("\n")[0] + "\n"
    assert code == case["exit"]
    assert err == case["stderr"]
    assert U.stdout_matches(case, out), out[:400]


def test_saturation_and_the_32_bit_unique_quirk():
    db, _ = M.parse_db(U.file_bytes(CASES, "db1.txt"))
    counts, st, err = M.count(db, [U.file_bytes(CASES, "polya.fa")])
    assert err is None and counts == [69976] and st["n_hits"] == 69976
    o16, _ = M.parse_argv(["-db", "d", "--unique", "--kmers", "f"])
    o32, _ = M.parse_argv(["-db", "d", "-32", "--unique", "--kmers", "f"])
    assert M.render(db, counts, st, o16, "d").endswith(b"only\t1\t1\t65535\n")
    assert M.render(db, counts, st, o32, "d").endswith(b"only\t1\t1\t69976\n")


@pytest.mark.parametrize("text", [
    b"#" + b"x" * 300 + b"\nn1\t2\tACGTA\tTACGT\n",            # a word and its reverse complement
    b"#" + b"x" * 300 + b"\nn1\t1\tACGTA\nn2\t1\tACGTA\n",      # the same word in two nodes
    b"#" + b"x" * 300 + b"\nn1\t3\tACGTA\tCCCCC\nn2\t1\tGGGTT\n",  # fewer k-mers than declared
    b"#" + b"x" * 300 + b"\nn1\t1\tACGTA\nn2\t1\tACG\n",        # a k-mer shorter than the word length
    b"#" + b"x" * 300 + b"\nn1\t1\tACGTA",                      # no final newline
    b"#" + b"x" * 300 + b"\nn1\t0\nn2\t1\tACGTA\n",             # the first node line gives no word length
])
def test_model_refuses_what_the_reference_misreads(text):
    with pytest.raises(M.Refused):
        M.parse_db(text)
