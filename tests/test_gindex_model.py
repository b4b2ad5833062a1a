"""tests/index_model.py against the reference's own `glistmaker --index` files (tests/golden/gindex_cases.json,
gindex_files.npz; made by tests/golden/make_golden_gindex.py): every byte, with the four undefined bytes of the file
block masked and nothing else."""
import hashlib

import pytest

import gindex_util as G
import index_model as IM

CASES, FILES = G.load()


@pytest.mark.parametrize("case", CASES["cases"], ids=[c["id"] for c in CASES["cases"]])
def test_model_reproduces_the_reference_index(case):
    texts = [G.file_bytes(CASES, n) for n in case["inputs"]]
    got = IM.masked(IM.index_bytes(texts, case["inputs"], case["k"], case["lo"], case["hi"]))
    assert len(got) == case["bytes"]
    if case["id"] in FILES:
        assert got == FILES[case["id"]]
    assert hashlib.sha256(got).hexdigest() == case["sha256"]


def test_the_goldens_cover_what_they_are_meant_to():
    by = {c["id"]: c for c in CASES["cases"]}
    bits = {cid: IM.parse(FILES[cid])["bits"] for cid in FILES}
    assert bits["pos255_k11"][2] == 8 and bits["pos256_k11"][2] == 9  # either side of a step of get_bitsize
    assert bits["three_files_k11"][0] == 2 and bits["two_files_k16"][0] == 1
    assert bits["many_k5"][1] == 9 and len(FILES["many_k11"]) == 72  # 300 subsequences; no word at all: a header alone
    cut = IM.parse(FILES["lowc_c2_k11"])
    assert cut["n_locations"] < len(cut["locations"])  # the cut-offs leave the location section whole (:568)
    assert by["big_k25"]["bytes"] > 2_000_000 and "big_k25" not in FILES
