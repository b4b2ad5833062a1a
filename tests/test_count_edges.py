"""The counts at the edges of u32 arithmetic against what the reference glistcompare made of them
(tests/golden/count_edges.json, tests/golden/make_golden_counts.py): ADD sums of exactly 2^32 (0: dropped) and 2^32 + 1,
N-way sums of eight 2^31, cutoffs up to 2^32 - 1, `-r <N>` near 2^32.  The CPU oracle first (it is what the large GPU
matrices of tests/test_pair_variants.py trust), then the C ABI and the drop-in CLI on the GPU."""
import functools
import hashlib
import os
import subprocess

import numpy as np
import pytest

import golden_util as G
import oracle_lib as O
from genometester4_amd.listio import write_list

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "genometester4_amd", "glistcompare")
GOLD = G.load_count_edges()
K = GOLD["word_length"]
OK_CASES = [c for c in GOLD["cases"] if c["exit"] == 0]
NWAY_REJECTED = [c for c in GOLD["cases"] if c["exit"] != 0 and c["id"].startswith("nway")]
NAME = {bit: "out_%d_%s.list" % (K, f) for bit, f in G.OP_FILES.items()}


@functools.lru_cache(maxsize=1)
def _lists():
    lists = G.count_edge_lists()
    assert len(lists) == GOLD["n_lists"]
    return lists


def _sha(data):
    return hashlib.sha256(data).hexdigest()


def _file(n, total, recs):
    return {"n_words": n, "total_count": total, "sha256": _sha(G.list_file_bytes(K, n, total, recs))}


def _indices(p):
    return [int(f[1:3]) for f in p["files"]]


def test_inputs_are_the_ones_the_reference_read(tmp_path):
    for j, rec in enumerate(_lists()):
        path = tmp_path / "l.list"
        write_list(str(path), rec, K)
        assert _sha(path.read_bytes()) == GOLD["inputs_sha256"]["L%02d.list" % j], j


def test_fixture_reaches_the_edges():
    ids = {c["id"] for c in OK_CASES}
    assert {"pair-u_c4294967295", "pair-i_r4294967290_c2147483648", "nway33-u_radd_c1", "nway33-i_c2147483648"} <= ids
    a, b = _lists()[:2]
    _, ia, ib = np.intersect1d(a["key"], b["key"], assume_unique=True, return_indices=True)
    sums = a["count"][ia].astype(np.uint64) + b["count"][ib].astype(np.uint64)
    assert (sums == 1 << 32).sum() > 100 and (sums == (1 << 32) + 1).sum() > 100


def _oracle(case):
    p = G.parse_argv(case["argv"])
    lists = [_lists()[j] for j in _indices(p)]
    if len(lists) == 2:
        res = O.compare(lists[0], lists[1], p["ops"], p["rule"], p["cutoff"], p["subtract"], p["count_override"])
        return {NAME[bit]: _file(*v) for bit, v in res.items()}
    out = {}
    for bit, fn in ((1, O.union_multi), (2, O.intersect_multi)):
        if p["ops"] & bit:
            rc, n, total, recs = fn(lists, p["cutoff"], p["rule"], p["count_override"])
            assert rc == 0, case["id"]
            out[NAME[bit]] = _file(n, total, recs)
    return out


@pytest.mark.parametrize("case", OK_CASES, ids=[c["id"] for c in OK_CASES])
def test_oracle_reproduces_reference(case):
    assert _oracle(case) == case["files"]


@pytest.mark.parametrize("case", NWAY_REJECTED, ids=[c["id"] for c in NWAY_REJECTED])
def test_oracle_rejects_what_the_reference_rejects(case):
    p = G.parse_argv(case["argv"])
    lists = [_lists()[j] for j in _indices(p)]
    fn = O.union_multi if p["ops"] & 1 else O.intersect_multi
    assert fn(lists, p["cutoff"], p["rule"], p["count_override"])[0] != 0


# ---------------------------------------------------------------- GPU


@pytest.fixture(scope="module")
def ctx():
    from genometester4_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def dev(ctx):
    return [ctx.upload(rec, K) for rec in _lists()]


def _gpu(ctx, dev, case):
    p = G.parse_argv(case["argv"])
    lists = [dev[j] for j in _indices(p)]
    out = {}
    if len(lists) == 2:
        st, res, _ = ctx.compare(lists[0], lists[1], p["ops"], p["rule"], p["cutoff"], p["subtract"], p["count_override"])
        for bit in st:
            out[NAME[bit]] = _file(st[bit][0], st[bit][1], res[bit].download())
        return out
    for bit, fn in ((1, ctx.union_multi), (2, ctx.intersect_multi)):
        if p["ops"] & bit:
            rc, n, total, res = fn(lists, p["cutoff"], p["rule"], p["count_override"])
            assert rc == 0, case["id"]
            out[NAME[bit]] = _file(n, total, res.download())
    return out


GPU_CASES = [(c, kway) for c in OK_CASES for kway in ((0, 1, 3) if c["id"].startswith("nway") and "-u" in c["argv"] else (1,))]


@pytest.mark.gpu
@pytest.mark.parametrize("case,kway", GPU_CASES, ids=["%s-kway%d" % (c["id"], k) for c, k in GPU_CASES])
def test_capi_reproduces_reference(ctx, dev, case, kway):
    try:
        ctx.set_option("kway", kway)
        got = _gpu(ctx, dev, case)
    finally:
        ctx.set_option("kway", 1)
    assert got == case["files"]


CLI_CASES = [c for c in GOLD["cases"] if c["id"] in ("pair-u-i-d-dd_c1", "pair-u_c4294967295", "pair-i_rmin_c2147483648",
                                                        "pair-du_r4294967290_c0", "pair-dd_rmax_c1", "pair-u_rmin_c1")]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CLI_CASES, ids=[c["id"] for c in CLI_CASES])
def test_cli_reproduces_reference(tmp_path, case):
    assert os.access(CLI, os.X_OK), "build it: make -C genometester4_amd/csrc"
    for j in {int(a[1:3]) for a in case["argv"] if a.endswith(".list")}:
        write_list(str(tmp_path / ("L%02d.list" % j)), _lists()[j], K)
    r = subprocess.run([CLI] + case["argv"], cwd=tmp_path, capture_output=True, timeout=300)
    assert (r.returncode, r.stdout.decode(), r.stderr.decode()) == (case["exit"], case["stdout"], case["stderr"])
    made = {}
    for name in sorted(os.listdir(tmp_path)):
        if name.startswith("out_"):
            data = (tmp_path / name).read_bytes()
            made[name] = {"n_words": int.from_bytes(data[16:24], "little"), "total_count": int.from_bytes(data[24:32], "little"),
                          "sha256": _sha(data)}
    assert made == case["files"]
