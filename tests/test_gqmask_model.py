"""tests/mask_model.py held to tests/golden/gqmask_cases.json, which tests/golden/make_golden_gqmask.py derived from the
reference's own `glistquery -s` sequence by sequence: every computed case byte for byte with its three counts, and the
malformed one up to the offending byte.  That licenses the model as the expectation of the GPU tests.  No GPU."""
import pytest

import gqmask_util as U
import mask_model as MM


def model(case):
    lst, fname, mm, pm, lo, hi, soft = U.parse(case["argv"])
    keys, counts, k = U.keys_counts(lst)
    return MM.mask_text(keys, counts, U.text_of(fname), k, mm, pm, lo, hi, soft)


def test_the_cases_the_issue_asks_for_are_there():
    ids = {c["id"] for c in U.CASES["cases"]}
    assert len(U.COMPUTED) >= 40 and len(U.MALFORMED) == 2 and len(U.REFUSED) >= 15
    assert {"k4_fa", "k9_fq", "k25_fa", "k9_crlf_fq", "pattern_k9", "pattern_k25", "zero_fa_min0", "bounds_min5_max9", "k9_fa_mm1", "k9_fq_mm2_p3", "k9_none_fa",
            "k9_all_fa", "k9_fa_soft", "err_gzip", "err_soft_alone"} <= ids
    assert any(c["counts"][1] == 0 for c in U.COMPUTED) and any(c["counts"][0] == c["counts"][1] > 0 for c in U.COMPUTED)


@pytest.mark.parametrize("case", U.COMPUTED, ids=lambda c: c["id"])
def test_model_gives_the_reference_s_masked_file(case):
    m = model(case)
    assert m.err is None
    assert m.text.decode("latin-1") == case["stdout"]
    assert list(m.counts) == case["counts"]


@pytest.mark.parametrize("case", U.MALFORMED, ids=lambda c: c["id"])
def test_model_masks_what_lies_in_front_of_a_reader_error(case):
    m = model(case)
    assert m.err is not None and m.err[0] == MM.ERR_PLUS
    assert m.text[:m.err[1]].decode("latin-1") == case["stdout"]
    assert list(m.counts) == case["counts"]


def test_backs_of_the_model():
    """a hit word over a cut: the piece it ends in reports the bases in front of the cut"""
    import numpy as np
    text = b">s\nAC\nGGA\n"  # k = 3: ACG, CGG (bases at 4, 6, 7) and GGA, all of different canonical forms
    keys = np.array([MM.read_bases(text, 3)[0][1]], dtype=np.uint64)
    m = MM.mask_text(keys, np.array([1], dtype=np.uint32), text, 3)
    assert m.hit.tolist() == [False, True, False] and m.text == b">s\nAN\nNNA\n" and m.counts == (3, 1, 3)
    assert [m.backs([c]) for c in (4, 5, 6, 7, 8)] == [[0, 0], [0, 1], [0, 1], [0, 2], [0, 0]]
    assert m.backs([5, 7]) == [0, 0, 2] and m.backs([]) == [0]
