"""tests/select_model.py -- the contract of glistcompare -u --min_lists M --max_lists X in numpy -- against what the
reference binary's own outputs imply (tests/golden/select_cases.json), and its two corner identities.  No GPU."""
import numpy as np
import pytest

import oracle_lib as O
import select_model as SM
import select_util as SU
from genometester4_amd.listio import make_records

INPUTS, CASES = SU.load_golden()


def test_the_goldens_cover_what_they_should():
    assert sorted({len(INPUTS[c["inputs"]][1]) for c in CASES}) == [2, 3, 5, 8, 9]
    assert {c["rule"] for c in CASES} == {"default", "max", "3"} and {c["cutoff"] for c in CASES} == {1, 3}
    assert all(int(l["count"].min()) >= 1 for _, lists in INPUTS.values() for l in lists)
    assert any(0 < c["n_words"] < len(O.union_multi(INPUTS[c["inputs"]][1])[3]) for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_model_reproduces_the_reference_derived_golden(case):
    _, lists = INPUTS[case["inputs"]]
    rule, ovr = SU.RULE_ARGS[case["rule"]]
    rc, n, t, rec = SM.select(lists, case["min_lists"], case["max_lists"], case["cutoff"], rule, ovr)
    assert (rc, n, t) == (0, case["n_words"], case["total_count"])
    assert rec.tobytes() == case["expected"].tobytes()


@pytest.mark.parametrize("name", sorted(INPUTS))
@pytest.mark.parametrize("rule,ovr,cutoff", [(0, 1, 1), (4, 1, 3), (7, 3, 1), (1, 1, 3)])
def test_everything_selected_is_the_union(name, rule, ovr, cutoff):
    _, lists = INPUTS[name]
    assert SM.select(lists, 1, len(lists), cutoff, rule, ovr)[3].tobytes() == O.union_multi(lists, cutoff, rule, ovr)[3].tobytes()


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_the_core_has_the_key_set_of_the_intersection(name):
    _, lists = INPUTS[name]
    n = len(lists)
    core = SM.select(lists, n, n)[3]
    inter = O.intersect_multi(lists)[3]
    assert len(core) and np.array_equal(core["key"], inter["key"])


def test_a_count_of_zero_does_not_hold_a_word():
    a = make_records([1, 5, 9], [2, 0, 1])
    b = make_records([5, 9, 11], [3, 4, 0])
    words, p = SM.presence([a, b])
    assert words.tolist() == [1, 5, 9] and p.tolist() == [1, 1, 2]
    assert SM.select([a, b], 2, 2)[3].tolist() == [(9, 5)]
    assert SM.select([a, b], 1, 1)[3].tolist() == [(1, 2), (5, 3)]  # 11 is in the union of no list: its only count is 0
    with pytest.raises(ValueError):
        SM.select([a, b], 0, 2)
    with pytest.raises(ValueError):
        SM.select([a, b], 2, 3)
    assert SM.select([a, b], 1, 2, rule=3)[0] != 0  # MIN: refused by the union
