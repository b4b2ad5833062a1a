"""glistcompare -mm N on the MI355X: every reference transcript of tests/golden/mm_cases.json replayed through the CLI
byte for byte, gt4hip_compare_mismatch against the numpy model (tests/mismatch_model.py) on random, planted and edge
inputs, live parity with the reference binary where it was built, and one full-size run checked by sampling."""
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import mismatch_model as MM
import mismatch_util as MU
from genometester4_amd.listio import make_records, read_list, write_list

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "genometester4_amd", "glistcompare")
REF = os.path.join(ROOT, "oracle", "_ref", "glistcompare")
with open(os.path.join(ROOT, "tests", "golden", "mm_cases.json")) as _f:
    GOLDEN = json.load(_f)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden_inputs():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_mm as MG
    d = tempfile.mkdtemp(prefix="gt4mm_gpu_")
    files = MG.build_inputs(sorted(GOLDEN["inputs"]), d)
    for fn, want in GOLDEN["input_files_sha256"].items():
        with open(os.path.join(d, fn), "rb") as f:
            assert hashlib.sha256(f.read()).hexdigest() == want, fn
    yield d, files
    shutil.rmtree(d, ignore_errors=True)


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=[c["id"] for c in GOLDEN["cases"]])
def test_cli_reproduces_reference(case, golden_inputs):
    d, files = golden_inputs
    run = tempfile.mkdtemp(dir=d)
    try:
        argv = ["../" + a if a in files.values() else a for a in case["argv"]]
        r = subprocess.run([CLI] + argv, cwd=run, capture_output=True, timeout=300)
        assert r.returncode == case["exit"], r.stderr.decode()
        assert r.stdout.decode() == case["stdout"]
        assert r.stderr.decode() == case["stderr"]
        assert sorted(os.listdir(run)) == sorted(case["files"])
        for name, want in case["files"].items():
            with open(os.path.join(run, name), "rb") as f:
                assert hashlib.sha256(f.read()).hexdigest() == want["sha256"], name
    finally:
        shutil.rmtree(run, ignore_errors=True)


@pytest.fixture(scope="module")
def ctx():
    from genometester4_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def _check(ctx, a, b, k, n, cutoff=1, subtract=False, ddiff=False):
    from genometester4_amd import capi
    ops = capi.OP_DIFF1 | (capi.OP_DIFF2 if ddiff else 0)
    exp = MM.compare_mismatch(a, b, k, n, cutoff, subtract, ddiff)
    da, db = ctx.upload(a, k), ctx.upload(b, k)
    st, out, timing = ctx.compare_mismatch(da, db, ops, n, cutoff=cutoff, subtract=subtract)
    for bit, rec in exp.items():
        got = out[bit].download()
        assert got.tobytes() == rec.tobytes(), (bit, len(got), len(rec))
        assert st[bit] == MM.totals(rec)
    cst, _, _ = ctx.compare_mismatch(da, db, ops, n, cutoff=cutoff, subtract=subtract, count_only=True)
    assert cst == st
    assert len(timing["level_ms"]) == min(n, 32)
    return timing


@pytest.mark.parametrize("k,n,cutoff,subtract,ddiff", [
    (4, 1, 1, False, True), (4, 2, 2, True, True), (5, 3, 1, False, False), (5, 2, 3, True, False),
    (6, 1, 0, False, True), (4, 6, 1, False, True), (5, 1, 4294967295, True, True), (6, 2, 2, False, True)])
def test_capi_dense_pairs_match_model(ctx, k, n, cutoff, subtract, ddiff):
    a, b = MU.dense_pair(100 + k * 10 + n, k, 0.3, 0.35)
    _check(ctx, a, b, k, n, cutoff, subtract, ddiff)


@pytest.mark.parametrize("k,n", [(13, 2), (25, 1), (25, 3), (31, 2), (32, 3)])
@pytest.mark.parametrize("subtract", [False, True])
def test_capi_planted_pairs_match_model(ctx, k, n, subtract):
    a, b = MU.planted_pair(7 * k + n, k, 2000 if n < 3 else 600)
    _check(ctx, a, b, k, n, 1, subtract, True)
    _check(ctx, a, b, k, n, 2, subtract, False)


def test_capi_edges(ctx):
    k = 5
    a, b = MU.dense_pair(9, k, 0.3, 0.3)
    empty = a[:0]
    for subtract in (False, True):
        _check(ctx, empty, b, k, 2, 1, subtract, True)   # empty A: diff2 looks up in nothing (the reference crashes)
        _check(ctx, a, empty, k, 2, 1, subtract, True)   # empty B: diff1 looks up in nothing
        _check(ctx, empty, empty, k, 1, 1, subtract, True)
        _check(ctx, a, b[:1], k, 2, 1, subtract, True)   # a 1-record B
        _check(ctx, a, a, k, 2, 1, subtract, True)       # all keys shared
    ka = np.arange(0, 1 << (2 * k), 2, dtype=np.uint64)
    kb = ka + np.uint64(1)
    a2 = make_records(ka, np.full(len(ka), 3, dtype=np.uint32))
    b2 = make_records(kb, np.full(len(kb), 2, dtype=np.uint32))
    _check(ctx, a2, b2, k, 2, 1, False, True)            # disjoint lists
    _check(ctx, a2, b2, k, 1, 3, True, True)             # -dd -du: diff2 drops a word with any variant in A


def test_capi_rejects_other_ops_and_zero_mismatches(ctx):
    from genometester4_amd import capi
    a, b = MU.dense_pair(1, 4)
    da, db = ctx.upload(a, 4), ctx.upload(b, 4)
    for ops in (capi.OP_UNION, capi.OP_INTRSEC | capi.OP_DIFF1, 0):
        with pytest.raises(capi.Gt4HipError) as e:
            ctx.compare_mismatch(da, db, ops, 1)
        assert e.value.code == capi.EINVAL
    with pytest.raises(capi.Gt4HipError) as e:
        ctx.compare_mismatch(da, db, capi.OP_DIFF1, 0)
    assert e.value.code == capi.EINVAL


def test_capi_caller_provided_outputs(ctx):
    from genometester4_amd import capi
    a, b = MU.planted_pair(3, 13, 3000)
    exp = MM.compare_mismatch(a, b, 13, 2, 1, False, True)
    da, db = ctx.upload(a, 13), ctx.upload(b, 13)
    o1, o2 = ctx.alloc(len(a), 13), ctx.alloc(len(b), 13)
    st, out, _ = ctx.compare_mismatch(da, db, capi.OP_DIFF1 | capi.OP_DIFF2, 2, out={4: o1, 8: o2})
    assert out[4] is o1 and out[8] is o2
    assert o1.download().tobytes() == exp[4].tobytes() and o2.download().tobytes() == exp[8].tobytes()
    small = ctx.alloc(len(a) - 1, 13)
    with pytest.raises(capi.Gt4HipError) as e:
        ctx.compare_mismatch(da, db, capi.OP_DIFF1, 1, out={4: small})
    assert e.value.code == capi.EINVAL


@pytest.mark.skipif(not os.path.exists(REF), reason="reference binary not built")
@pytest.mark.parametrize("k,n", [(25, 1), (13, 2)])
def test_cli_live_parity_with_reference(k, n):
    a, b = MU.planted_pair(1000 + k, k, 100_000, shared=0.5, planted=0.3)
    d = tempfile.mkdtemp(prefix="gt4mm_live_")
    try:
        write_list(os.path.join(d, "a.list"), a, k)
        write_list(os.path.join(d, "b.list"), b, k)
        for tool, sub in ((REF, "ref"), (CLI, "gpu")):
            os.mkdir(os.path.join(d, sub))
            r = subprocess.run([tool, "../a.list", "../b.list", "-dd", "-mm", str(n)], cwd=os.path.join(d, sub),
                               capture_output=True, timeout=600)
            assert r.returncode == 0, r.stderr.decode()
        for name in ("out_%d_%d_diff1.list" % (k, n), "out_%d_%d_diff2.list" % (k, n)):
            with open(os.path.join(d, "ref", name), "rb") as f1, open(os.path.join(d, "gpu", name), "rb") as f2:
                assert f1.read() == f2.read(), name
    finally:
        shutil.rmtree(d, ignore_errors=True)


def test_full_size_planted(ctx):
    """2 x 2e8 records, k = 25 (tools/mm_bench.py's workload): A = S + PA, B = S + PB + one-mismatch neighbours of 2e5
    words of PA.  -mm 1 and -mm 2 are checked on a sample of the pre-pass table, kept and dropped words, by host
    searchsorted on the downloaded lists; the totals against the output itself."""
    from genometester4_amd import capi
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import mm_bench
    k = 25
    rng = np.random.default_rng(78)
    A, B, src = mm_bench.planted_device_pair(ctx, 200_000_000, 10_000_000, 200_000, k)
    a_host, b_host = A.download(), B.download()
    # every count is >= 1 = cutoff: the pre-pass table is A without the keys B shares
    table = a_host[~MM.present(b_host["key"], a_host["key"])]
    pick = np.concatenate([rng.choice(len(table), 10_000, replace=False), np.searchsorted(table["key"], src[:2000])])
    sample = table[np.unique(pick[pick < len(table)])]
    for nmm in (1, 2):
        st, out, timing = ctx.compare_mismatch(A, B, capi.OP_DIFF1, nmm)
        got = out[4].download()
        out[4].free()
        assert st[4] == MM.totals(got)
        assert timing["prepass_words"][0] == len(table)
        exp = MM.fetch(sample, k, nmm, 1, b_host["key"], None, False)
        kept = MM.present(got["key"], sample["key"])
        assert np.array_equal(sample["key"][kept], exp["key"])
        assert 0 < kept.sum() < len(sample)
