"""tests/query_model.py held to the reference's own transcripts (tests/golden/gquery_cases.json): every recorded
lookup on one list (-q / -f / -s / -l with -mm, -p, -min, -max, --all, --3p, --5p) and the statistics commands must
come out of the numpy restatement byte for byte, so that the GPU tests on large inputs have an independent yardstick.
No GPU, no binary."""
import numpy as np
import pytest

import gquery_util as U
import query_model as M

LISTS = U.lists()


def _query_cases():
    for c in U.CASES["cases"]:
        p = U.parse(c["argv"])
        if len(p["lists"]) == 1 and not p["other"] and (p["q"] or p["f"] or p["s"] or p["l"]) and p["mm"] + p["p"] <= LISTS[p["lists"][0][:-5]][1]:
            if p["l"] and not p["mm"]:
                continue  # the zipper: tests/test_query_forms.py
            if p["f"] and p["f"] not in U.CASES["files"] or p["s"] and p["s"] not in U.CASES["files"]:
                continue
            yield c, p


def _words(p, k):
    if p["q"] is not None:
        q = p["q"]
        if len(q) < k or (len(q) > k and not (p["use_3p"] or p["use_5p"])):
            return [], 1
        return [M.string_to_word(q[len(q) - k:] if len(q) > k and p["use_3p"] else q, k)], 0
    if p["f"]:
        return M.query_file_words(U.CASES["files"][p["f"]], k, p["use_3p"], p["use_5p"])
    if p["s"]:
        w, rc = M.fasta_words(U.CASES["files"][p["s"]], k)
        return w, rc & 0xFF
    return [int(x) for x in LISTS[p["l"][:-5]][0]["key"]], 0


@pytest.mark.parametrize("case,p", list(_query_cases()), ids=lambda x: x["id"] if "id" in x else "")
def test_model_prints_what_the_reference_printed(case, p):
    rec, k = LISTS[p["lists"][0][:-5]]
    keys, counts = rec["key"].astype(np.uint64), rec["count"].astype(np.uint32)
    words, rc = _words(p, k)
    assert rc == case["exit"]
    if p["all"]:
        out = "".join(M.search_one_word(keys, counts, w, k, p["mm"], p["p"], p["min"], p["max"], True) for w in words)
    else:
        w = np.array(words, dtype=np.uint64)
        val, found = M.lookup_np(keys, counts, w, k, p["mm"], p["p"])
        cq = M.canonical_np(w, k) if len(w) else w
        out = []
        for q, v, f in zip(cq, val, found):
            if f:
                if p["min"] <= int(v) <= p["max"]:
                    out.append("%s\t%u\n" % (M.word_to_string(int(q), k), v))
            elif not p["min"]:
                out.append("%s\t0\n" % M.word_to_string(int(q), k))
        out = "".join(out)
    U.check_stdout(case, out.encode("latin-1"))


def test_the_cases_cover_what_they_must():
    ids = {c["id"] for c in U.CASES["cases"]}
    assert len(ids) == len(U.CASES["cases"]) >= 150
    ks = {LISTS[U.parse(c["argv"])["lists"][0][:-5]][1] for c, _ in _query_cases()}
    assert {4, 16, 25, 32} <= ks
    assert {U.parse(c["argv"])["mm"] for c, _ in _query_cases()} >= {0, 1, 2, 3}
    assert all(c["exit"] >= 0 for c in U.CASES["cases"])


@pytest.mark.parametrize("name", ["A8", "R1", "W1", "H1", "MEDE", "MED1", "MED1B", "MEDQ", "MEDW", "G25"])
def test_model_statistics(name):
    rec, k = LISTS[name]
    case = {c["id"]: c for c in U.CASES["cases"]}
    total = int(rec["count"].astype(np.uint64).sum())
    gmin, gmax, med = M.median_lines(rec["count"], total)
    last = case["median_" + name]["stdout"].splitlines()[-1]
    assert last == "Min %u Max %u Median %u Average %.2f" % (gmin, gmax, med, total / len(rec))
    gc = M.gc_bases(rec["key"], rec["count"], k)
    assert case["gc_" + name]["stdout"] == "GC\t%g\n" % (gc / (total * k))


def test_variant_order_and_count():
    for k, n_mm, pm_3 in ((4, 2, 0), (4, 4, 0), (8, 2, 3), (16, 3, 10), (12, 1, 11)):
        m = M.variant_masks(k, n_mm, pm_3)
        assert len(m) == len(set(m)) == M.n_variants(k, n_mm, pm_3)
        assert sorted(m) == sorted(int(x) for x in M.masks_np(k, n_mm, pm_3))
        assert all(x & ((1 << (2 * pm_3)) - 1) == 0 for x in m)
