"""tests/maker_model.py against the reference glistmaker's own files (tests/golden/gmaker_cases.json, made by
tests/golden/make_golden_gmaker.py from oracle/_ref/glistmaker): the model reproduces every recorded .list byte for
byte, and names the reference's reader errors.  No GPU."""
import pytest

import gmaker_util as U
import maker_model as M

CASES = U.load_cases()
WITH_LIST = [c for c in CASES["cases"] if c["output"]]


def _inputs(argv):
    return [a for a in argv if a in CASES["files"]]


def _k(argv):
    return int(argv[[i for i, a in enumerate(argv) if a in ("-w", "--wordlength")][0] + 1])


@pytest.mark.parametrize("case", WITH_LIST, ids=lambda c: c["id"])
def test_model_reproduces_the_reference_list(case):
    assert len(WITH_LIST) >= 40 and case["exit"] == 0
    data = M.list_bytes([U.file_bytes(CASES, n) for n in _inputs(case["argv"])], _k(case["argv"]))
    if "list_hex" in case:
        assert data.hex() == case["list_hex"]
    else:
        assert (len(data), U.sha(data)) == (case["list_bytes"], case["list_sha256"])


def test_cutoffs_do_nothing_to_a_list():
    by_id = {c["id"]: c for c in CASES["cases"]}
    assert by_id["cutoffs_k5"]["list_hex"] == by_id["multi_fa_k5"]["list_hex"]


def test_model_names_the_reader_errors():
    by_id = {c["id"]: c for c in CASES["cases"]}
    words, err = M.read_words(U.file_bytes(CASES, "bad_start.fa"), 4)
    assert err == (M.ERR_START, 0) and "invalid start tag 'A'" in by_id["bad_start_k4"]["stderr"]
    text = U.file_bytes(CASES, "no_plus.fq")
    words, err = M.read_words(text, 4)
    at = text.index(b"\n", 4) + 1
    assert err == (M.ERR_PLUS, at)
    assert "tag '+' missing, found 'I' instead at %d\n" % (at - 1) in by_id["no_plus_k4"]["stderr"]
    assert M.read_words(b"@r\nACGT\n+\nIIII\nX", 2)[1] == (M.ERR_AT, 15)
    assert M.read_words(b"@r\nACGT\n+", 2)[1] == (M.ERR_PLUS_EOF, 9)
    assert M.read_words(b"@r\nACGT\n", 2)[1] == (M.ERR_PLUS, 8)
    assert M.read_words(b"@r\nACGT", 2) == ([0b0001, 0b0110, 0b0001], None)  # AC, CG, GT; GT's reverse complement AC is the smaller


def test_forward_words_and_a_nul():
    assert M.read_words(b">x\nAC\nGT\x00ACGT", 2, canonize=False) == ([0b0001, 0b0110, 0b1011], None)
    assert M.read_words(b">x\nACNGT>name ACGT\nTT", 2, canonize=False)[0] == [0b0001, 0b1011, 0b1111]
