"""tests/caller_model.py against the reference's transcripts (tests/golden/caller_cases.json): every --runs 0 case and
every trained case of at most 500 markers byte for byte, the "Iteration" values of -D -D included."""
import pytest

import caller_model as M
import caller_util as U

CASES = U.load_cases()
REPLAYED = [c for c in CASES["cases"] if c["device"] and (not c["trained"] or c["markers"] <= 500)]


@pytest.mark.parametrize("case", REPLAYED, ids=lambda c: c["id"])
def test_model_replays_the_golden(case):
    assert len(REPLAYED) >= 40 and sum(c["trained"] for c in REPLAYED) >= 12
    name = case["argv"][-1]
    r = M.run_cli(case["argv"], U.file_bytes(CASES, name))
    assert r.exit == case["exit"] and r.stderr_lines == case["stderr_lines"]
    assert U.stdout_matches(case, r.stdout), r.stdout[:300]
    if case["trained"]:
        assert r.iterations == case["iterations"] and len(r.iterations) > 7


def test_goldens_cover_what_they_must():
    cases = [c for c in CASES["cases"] if c["device"]]
    trained = [c for c in cases if c["trained"]]
    assert len(cases) >= 40 and len(trained) >= 12 and sum(c["markers"] <= 3 for c in trained) <= 1
    assert all(c["markers"] <= 6500 for c in trained)
    argvs = [" ".join(c["argv"]) for c in cases]
    for needle in ("--model diploid", "--model haploid", "--alternatives", "--non_canonical", "--prob_cutoff 0.99", "--header", "--info", "--no_genotypes",
                   "--params", "--coverage", "pairs2.txt", "pairs3.txt", "fem.txt", "male.txt", "edge.txt"):
        assert any(needle in a for a in argvs), needle
    by_id = {c["id"]: c for c in cases}
    nc = by_id["r0_fem_no_coverage_all_nc"]  # without --coverage, --params or a training lambda is 0: every marker is NC
    out = M.run_cli(nc["argv"], U.file_bytes(CASES, "fem.txt")).stdout
    assert U.stdout_matches(nc, out) and all(b"\tNC\t\t" in l for l in out.split(b"\n")[:-1]) and out.count(b"\n") == nc["markers"] - 30  # (a female's 30 Y markers are not printed)
    edge = by_id["r0_edge_alt_header_info"]["stdout"]
    assert "X:7\tNC\t\t17000\t3\t-nan" in edge and "1:200\tNC\t\t0\t0" in edge and "3:500\t" in edge and "chr1" not in edge and "#Sex" in edge


def test_fast_and_plain_objective_agree_bit_for_bit():
    text = U.file_bytes(CASES, "auto.txt")
    pairs = [(int(l.split(b"\t")[2]), int(l.split(b"\t")[3])) for l in text.split(b"\n") if l]
    model = M.Model(0.0547219, 4.2603e-05, 0.014934, 0.985023, 20.0, 65.48, -0.6792684, 0.3)
    run = type("R", (), dict(iterations=[]))()
    tr = M.Training(pairs, M.F(0.3), M.F(20.0), 16, run)
    total = 0.0
    for t in tr.logs(model):
        total += t
    s, bound = M.mlogl(model, pairs)
    assert s == -total and 0 < bound < 1e-8


def test_float_rounding_helper():
    assert M.F(0.1) == 0.10000000149011612 and M.F(1e40) == float("inf") and M.F(-1e40) == float("-inf") and M.F(1e-50) == 0.0
