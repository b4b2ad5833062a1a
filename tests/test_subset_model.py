"""tests/subset_model.py without a GPU: its serial walk is the reference's loop (every list of
tests/golden/subset_cases.json), and its parallel iteration -- what gt4hip_list_subset runs -- reaches the serial walk's
list within items + 1 passes."""
import base64
import json
import os
import sys

import numpy as np
import pytest

import subset_model as SM
from genometester4_amd.listio import RECORD_DTYPE, parse_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_subset as MG  # noqa: E402

METHODS = {"rand": SM.RAND, "rand_unique": SM.RAND_UNIQUE, "rand_weighted_unique": SM.RAND_WEIGHTED_UNIQUE}


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "subset_cases.json")) as f:
        return json.load(f)


def _subset_args(argv):
    i = argv.index("--subset") if "--subset" in argv else argv.index("-ss")
    seed = int(argv[argv.index("--seed") + 1])
    return METHODS[argv[i + 1]], int(argv[i + 2]), seed


def test_golden_covers_what_it_must(golden):
    cases = [c for c in golden["cases"] if c["exit"] == 0]
    args = [_subset_args(c["argv"]) for c in cases]
    assert {a[0] for a in args} == {0, 1, 2}
    assert {a[2] for a in args} >= {0, 1, 7, -2, (1 << 32) + 7, (1 << 31) - 1}
    assert {MG.INPUTS[c["inputs"][0]][3] for c in cases if MG.INPUTS[c["inputs"][0]][0] == "list"} == {1, 13, 25, 32}
    assert {a[1] for a, c in zip(args, cases) if c["inputs"] == ["u300"]} >= {0, 1, 100, 299, 300}
    assert any("--stream" in c["argv"] for c in cases) and any("-D" in c["argv"] for c in cases)
    assert any("dir/name" in c["argv"] for c in cases) and any(c["inputs"] == ["Ia_6"] for c in cases)
    assert len([c for c in golden["cases"] if c["exit"] == 1]) >= 5
    assert len({c["id"] for c in golden["cases"]}) == len(golden["cases"])


def test_serial_walk_reproduces_every_golden_list(golden):
    checked = 0
    for c in golden["cases"]:
        if c["exit"] != 0 or MG.INPUTS[c["inputs"][0]][0] != "list":
            continue
        rec, k = MG.input_records(c["inputs"][0])
        method, size, seed = _subset_args(c["argv"])
        (name, data), = c["files"].items()
        data = base64.b64decode(data)
        h = parse_header(data[:48])
        want = np.frombuffer(data[48:], dtype=RECORD_DTYPE)
        got = SM.serial_walk(rec, method, size, SM.state48(seed))
        assert name.endswith("_subset_%d.list" % k), c["id"]
        assert got.tobytes() == want.tobytes(), c["id"]
        assert (h["n_words"], h["total_count"], h["word_length"]) == (len(got), int(got["count"].astype(np.uint64).sum()), k), c["id"]
        checked += 1
    assert checked >= 60


def test_seed_uses_its_low_32_bits(golden):
    by_id = {c["id"]: c for c in golden["cases"]}
    assert by_id["u300_unique_100_seed4294967303"]["files"] == by_id["u300_unique_100_seed7"]["files"]
    assert by_id["u300_unique_100_seed1"]["files"] != by_id["u300_unique_100_seed7"]["files"]
    assert SM.state48((1 << 32) + 7) == SM.state48(7) == (7 << 16) | 0x330E
    assert SM.state48(-2) == (0xFFFFFFFE << 16) | 0x330E


def test_draws_and_jump_ahead():
    x0 = SM.state48(7)
    x, xs = x0, []
    for _ in range(1000):
        x = (SM.LCG_A * x + SM.LCG_C) & SM.LCG_MASK
        xs.append(x)
    assert [int(v) for v in SM.states(x0, 1000)] == xs
    assert SM.draws(x0, 3).tolist() == [v / 2.0 ** 48 for v in xs[:3]]
    for pos in (0, 1, 2, 63, 64, 999, 1000):
        assert SM.state_at(x0, pos) == ([x0] + xs)[pos]
    # the period is 2^48
    assert SM.state_at(x0, 1 << 48) == x0 and SM.state_at(x0, (1 << 48) + 5) == xs[4]


def test_parallel_iteration_equals_the_serial_walk():
    """a few thousand random small cases of the three methods, sizes from 0 to all, shortfalls included"""
    rng = np.random.default_rng(20261019)
    n_cases = n_short = 0
    for method in (SM.RAND, SM.RAND_UNIQUE, SM.RAND_WEIGHTED_UNIQUE):
        for _ in range(1000):
            n = int(rng.integers(0, 40))
            max_count = int(rng.choice([1, 3, 30]))
            rec = SM.make_list(int(rng.integers(0, 1 << 30)), n, 13, max_count)
            if n and rng.random() < 0.2:
                rec["count"][rng.integers(0, n, size=2)] = 0  # records that own no item
            it = SM.Items(rec, method)
            size = int(rng.integers(0, it.items + 3))
            x0 = SM.state48(int(rng.integers(-5, 1 << 33)))
            try:
                want = SM.serial_walk(rec, method, size, x0)
            except SM.Shortfall as e:
                with pytest.raises(SM.Shortfall) as p:
                    SM.parallel_iteration(rec, method, size, x0)
                assert p.value.reached == e.reached
                n_short += 1
                continue
            got, passes = SM.parallel_iteration(rec, method, size, x0)
            assert got.tobytes() == want.tobytes(), (method, n, size, x0)
            assert passes <= it.items + 1
            assert passes >= 1 or n == 0 or size == 0
            n_cases += 1
    assert n_cases > 1500 and n_short > 50


def test_parallel_iteration_at_a_few_thousand_items():
    rec = SM.make_list(77, 3000, 25, 30)
    for method, size in ((SM.RAND_UNIQUE, 1000), (SM.RAND_WEIGHTED_UNIQUE, 600), (SM.RAND, 20000)):
        want = SM.serial_walk(rec, method, size, SM.state48(3))
        got, passes = SM.parallel_iteration(rec, method, size, SM.state48(3))
        assert got.tobytes() == want.tobytes()
        assert 2 <= passes <= SM.Items(rec, method).items + 1
