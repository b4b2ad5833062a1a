"""The query and statistics kernels (gt4hip_query.hip) may not spill or touch scratch memory, and moving the bucket
index into gt4hip_index.h must leave the -mm kernels of gt4hip_mismatch.hip with the registers and LDS they had
(tools/kernel_resources.py; hipcc cross-compiles gfx950 without a GPU)."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# (VGPR, SGPR, LDS bytes) of gt4hip_mismatch.hip's kernels before the index moved into its own header
MM_BEFORE = {
    "k_index_build": (8, 25, 0), "k_prepass": (18, 54, 0), "k_tile_count": (18, 42, 16), "k_tile_scan": (36, 51, 136), "k_decide": (7, 26, 0),
    "k_level<false>": (38, 93, 0), "k_level<true>": (40, 94, 0), "k_scatter<true, false>": (30, 64, 16), "k_scatter<false, false>": (30, 64, 16),
    "k_scatter<false, true>": (35, 68, 16),
}


@pytest.fixture(scope="module")
def K():
    if not shutil.which("hipcc"):
        pytest.skip("hipcc not on PATH")
    import kernel_resources
    return kernel_resources


def test_query_kernels_do_not_spill(K):
    rows = K.table("gt4hip_query.hip")
    names = [r["name"] for r in rows]
    for want in ("k_query<false>", "k_query<true>", "k_query_exact", "k_query_hits<false, false>", "k_query_hits<true, false>", "k_query_hits<false, true>",
                 "k_query_hits<true, true>", "k_count_stats", "k_count_split", "k_count_histogram<true>", "k_count_histogram<false>", "k_gc"):
        assert want in names, names
    bad = [(r["name"], r["vspill"], r["sspill"], r["scratch"]) for r in rows if r["vspill"] or r["sspill"] or r["scratch"]]
    assert not bad, bad
    assert all(r["vgpr"] <= 64 for r in rows), rows  # eight wavefronts per SIMD, as the grids are sized for


# (VGPR, LDS bytes) of k_query_all<FILL> and k_query_loc<FILL> before they became k_query_hits<FILL, LOC>: ceilings
HITS_BEFORE = {
    "k_query_hits<false, false>": (28, 16), "k_query_hits<true, false>": (36, 16), "k_query_hits<false, true>": (36, 48), "k_query_hits<true, true>": (54, 48),
}


def test_the_merged_hit_kernel_costs_no_more_than_its_two_parents(K):
    rows = {r["name"]: (r["vgpr"], r["lds"]) for r in K.table("gt4hip_query.hip")}
    for name, (vgpr, lds) in HITS_BEFORE.items():
        assert rows[name][0] <= vgpr and rows[name][1] <= lds, (name, rows[name])


def test_mismatch_kernels_keep_their_resources(K):
    rows = {r["name"]: (r["vgpr"], r["sgpr"], r["lds"]) for r in K.table("gt4hip_mismatch.hip")}
    assert rows == MM_BEFORE
    assert all(r["vspill"] == 0 and r["scratch"] == 0 for r in K.table("gt4hip_mismatch.hip"))
