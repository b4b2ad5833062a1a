"""tests/locations_model.py, the Python restatement of glistquery on a GT4I index, reproduces every transcript of the
reference in tests/golden/gqloc_cases.json: --files, --sequences, the dump with locations, and -q / -f / -s / -l with
and without --locations, the sticky REVERSE flag among them.  No device, no binary."""
import shutil

import pytest

import gqloc_util as U
import locations_model as L


@pytest.fixture(scope="module")
def workdir():
    d = U.make_workdir(built="model")
    yield d
    shutil.rmtree(d, ignore_errors=True)


@pytest.mark.parametrize("case", U.CASES["cases"], ids=lambda c: c["id"])
def test_model_reproduces_the_reference(case, workdir):
    out, rc = L.replay(case["argv"], workdir)
    assert rc == case["exit"]
    U.check_stdout(case, out.encode("latin-1"))


def test_the_cases_cover_what_they_should():
    ids = [c["id"] for c in U.CASES["cases"]]
    assert len(ids) >= 90 and len(set(ids)) == len(ids)
    for c in U.CASES["cases"]:
        if "--locations" in c["argv"] and not c["id"].startswith("dump_"):
            assert c["id"] + "_plain" in ids  # the same argv without --locations
    sticky = next(c for c in U.CASES["cases"] if c["id"] == "f_q_rev_fwd_mm0")["stdout"].split("\n")
    flags = [l.split("\t")[2] for l in sticky if l[:1] in "ACGT" and l.count("\t") == 2]
    assert flags == sorted(flags) and flags[0] == "0" and flags[-1] == "1"  # REVERSE rises once and stays


def test_sticky_flag_and_strands():
    ix = L.Index(U.GFILES["multi_k11"])
    fwd, rev = "ACGTTGCAAGG", "CCTTGCAACGT"
    s = L.Searcher(ix)
    a = s.search(L.M.string_to_word(fwd, 11))
    b = s.search(L.M.string_to_word(rev, 11))
    c = s.search(L.M.string_to_word(fwd, 11))
    assert a.split("\n")[0] == fwd + "\t1\t0" and b.split("\n")[0] == fwd + "\t1\t1" and b == c
    assert a.split("\n")[1].endswith("\t0") and b.split("\n")[1].endswith("\t1")
