"""tests/pairwise_model.py -- the contract of glistcompare --pairwise in numpy -- against what the reference binary printed
for every pair of lists (tests/golden/pairwise_cases.json), and the identities the derived numbers rest on.  No GPU."""
import numpy as np
import pytest

import pairwise_model as PM
import pairwise_util as PU
from genometester4_amd.listio import make_records

CASES = PU.load_golden()


def test_the_goldens_cover_what_they_should():
    assert {c["word_length"] for c in CASES} == {1, 16, 25, 32}
    assert all(2 <= len(c["records"]) <= 6 for c in CASES) and {len(c["records"]) for c in CASES} >= {2, 6}
    assert all(len(c["pairs"]) == len(c["records"]) * (len(c["records"]) - 1) // 2 for c in CASES)
    assert all(len(l) == 0 or int(l["count"].min()) >= 1 for c in CASES for l in c["records"])
    shapes = next(c for c in CASES if c["id"] == "k25_n5_shapes")["records"]
    assert any(len(l) == 0 for l in shapes) and shapes[0].tobytes() == shapes[1].tobytes() and not np.isin(shapes[0]["key"], shapes[3]["key"]).any()
    top = next(c for c in CASES if c["id"] == "k16_n3_top")
    assert max(int(l["count"].max()) for l in top["records"]) == 0xffffffff and all(p["intersection"][1] > 1 << 32 for p in top["pairs"])
    assert any(int(l["key"].max()) == (1 << 64) - 1 for c in CASES if c["word_length"] == 32 for l in c["records"])


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_model_reproduces_the_reference(case):
    shared, min_total = PM.pairwise(case["records"])
    want_shared, want_min = PU.golden_matrices(case)
    assert np.array_equal(shared, want_shared) and np.array_equal(min_total, want_min)
    assert shared.dtype == min_total.dtype == np.uint64
    for p in case["pairs"]:
        i, j = p["i"], p["j"]
        assert PM.union_size(shared, i, j) == p["union"][0]
        assert int(shared[i][i]) - int(shared[i][j]) == p["difference_ij"][0]
        assert int(shared[j][j]) - int(shared[i][j]) == p["difference_ji"][0]
    for d in case["diagonal"]:
        l = case["records"][d["i"]]
        assert d["intersection"] == [len(l), int(l["count"].astype(np.uint64).sum())]


def test_a_count_of_zero_is_absence():
    a = make_records([1, 5, 9], [2, 0, 1])
    b = make_records([5, 9, 11], [3, 4, 0])
    shared, min_total = PM.pairwise([a, b])
    assert shared.tolist() == [[2, 1], [1, 2]] and min_total.tolist() == [[3, 1], [1, 7]]
    assert PM.union_size(shared, 0, 1) == 3 and PM.jaccard(shared, 0, 1) == 1 / 3


def test_sums_beyond_32_bits_and_empty_lists():
    top = 0xffffffff
    a = make_records([1, 2, 3], [top, top, top])
    e = a[:0]
    shared, min_total = PM.pairwise([a, a, e])
    assert min_total[0][1] == 3 * top and min_total[0][1] > 1 << 32
    assert shared[2].tolist() == [0, 0, 0] and shared[:, 2].tolist() == [0, 0, 0] and PM.jaccard(shared, 2, 2) == 0.0
    shared, min_total = PM.pairwise([e])
    assert shared.tolist() == [[0]] and min_total.tolist() == [[0]]


def test_the_transcript():
    a = make_records([1, 5, 9], [2, 4, 1])
    b = make_records([5, 9, 11], [3, 4, 6])
    shared, min_total = PM.pairwise([a, b])
    assert PM.transcript(["x.list", "d/y.list"], shared, min_total) == (
        "#I\tJ\tLIST_I\tLIST_J\tSHARED\tMIN_TOTAL\tUNION\tJACCARD\n"
        "0\t0\tx.list\tx.list\t3\t7\t3\t1.000000\n"
        "0\t1\tx.list\td/y.list\t2\t4\t4\t0.500000\n"
        "1\t1\td/y.list\td/y.list\t3\t13\t3\t1.000000\n")
