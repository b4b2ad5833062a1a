"""tests/seqprofile_model.py against what the reference's own `glistquery -s` prints sequence by sequence
(tests/golden/gqseq_cases.json): every computed case, stdout byte for byte and the unfiltered rows.  No GPU.  The fixture
itself is checked for what its maker promises: a case where every sequence hits and one with a sequence that does not."""
import numpy as np
import pytest

import gqseq_util as U
import seqprofile_model as SP

CASES = U.CASES["cases"]
COMPUTED = [c for c in CASES if c["kind"] == "computed"]
LISTS = U.lists()


def test_the_fixture_covers_what_it_promises():
    assert len(CASES) >= 36 and len(COMPUTED) >= 30
    assert any(c["rows"] and all(r[2] > 0 for r in c["rows"]) for c in COMPUTED)
    assert any(any(r[2] == 0 for r in c["rows"]) for c in COMPUTED)
    assert any(r[3] > 1 << 32 for c in COMPUTED for r in c["rows"])  # a SUM that needs 64 bits
    assert any(r[0] == "" for c in COMPUTED for r in c["rows"])      # an empty name
    assert {k for _, k in LISTS.values()} >= {4, 9, 25}
    assert sum(c["kind"] == "argv" for c in CASES) >= 12 and sum(c["kind"] == "malformed" for c in CASES) == 1
    assert all(len(t) < 2000 for t in U.CASES["files"].values())


@pytest.mark.parametrize("case", COMPUTED, ids=lambda c: c["id"])
def test_the_model_reproduces_the_reference(case):
    lst, fname, mm, pm, lo, hi, min_hits = U.parse(case["argv"])
    rec, k = LISTS[lst]
    text = U.CASES["files"][fname].encode("latin-1")
    keys, counts = rec["key"].astype(np.uint64), rec["count"].astype(np.uint32)
    assert SP.stdout_of(keys, counts, text, k, mm, pm, lo, hi, min_hits).decode("latin-1") == case["stdout"]
    names, rows = SP.profile_text(keys, counts, text, k, mm, pm, max(lo, 1), hi)
    assert [[n.decode("latin-1")] + [int(x) for x in r] for n, r in zip(names, rows)] == case["rows"]
