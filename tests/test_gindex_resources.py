"""The pair sort and the index fold added to gt4hip_sort.hip and the location kernels added to gt4hip_maker.hip may not spill or touch scratch memory, the pair scatter
kernel must still fit two workgroups on a CU (four wavefronts per SIMD, LDS of the keys-only kernel), and the kernels
that were there before keep the vector registers, LDS and occupancy they had (tools/kernel_resources.py; hipcc cross-compiles gfx950
without a GPU)."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# (VGPR, LDS bytes, wavefronts per SIMD) before the pair sort and the location kernels were added; scalar registers move
# with the compiler and are not pinned.  The figures are those of the ROCm release the project is built with: a compiler
# update may move them without anything being wrong, and they are then recorded anew.
SORT_BEFORE = {
    "k_radix_hist": (78, 16384, 6), "k_radix_bases": (26, 64, 8), "k_fold_count": (70, 36, 7), "k_fold_records": (70, 72, 7),
    "k_radix_scatter<9>": (99, 79912, 4), "k_radix_scatter<8>": (100, 72728, 4),
}
# The vector registers of k_mk_codes (55, 52) and k_mk_emit (41, 122) were recorded anew when their bodies came to be shared
# with k_mk_events and k_mk_emit_loc (tile_head, load_word_ends, for_each_word): LDS and occupancy are what they were, and the
# extraction was measured against the commit before (profiles/maker/README.md).
MAKER_BEFORE = {
    "k_index_build": (8, 0, 8), "k_tile_count": (18, 16, 8), "k_tile_scan": (36, 136, 8), "k_mk_summary": (47, 48, 8), "k_mk_state_scan": (36, 12288, 8),
    "k_mk_codes<true>": (61, 4144, 7), "k_mk_codes<false>": (59, 4144, 7), "k_mk_emit<false>": (61, 16, 8), "k_mk_emit<true>": (91, 32784, 4),
}
# the location kernels, as they stand since they share those bodies (no occupancy below what it was before: 8, 6, 8, 7, 4, 4, 8)
MAKER_NEW = {
    "k_mk_events<false, false>": (36, 48, 8), "k_mk_events<false, true>": (70, 64, 7), "k_mk_events<true, false>": (40, 32, 8), "k_mk_events<true, true>": (72, 32, 7),
    "k_mk_emit_loc<2>": (123, 32, 4), "k_mk_emit_loc<3>": (123, 32, 4), "k_pack_locations": (10, 0, 8),
}
NEW = ("k_radix_scatter_pairs<9>", "k_radix_scatter_pairs<8>", "k_index_sums", "k_index_scan", "k_index_write")
NEW_MAKER = tuple(MAKER_NEW)


@pytest.fixture(scope="module")
def K():
    if not shutil.which("hipcc"):
        pytest.skip("hipcc not on PATH")
    import kernel_resources
    return kernel_resources


@pytest.fixture(scope="module")
def sort_rows(K):
    return {r["name"]: r for r in K.table("gt4hip_sort.hip")}


def test_new_kernels_do_not_spill(sort_rows):
    for name in NEW:
        assert name in sort_rows, sorted(sort_rows)
        r = sort_rows[name]
        assert (r["vspill"], r["sspill"], r["scratch"]) == (0, 0, 0), r


def test_new_maker_kernels_do_not_spill(K):
    rows = {r["name"]: r for r in K.table("gt4hip_maker.hip")}
    for name in NEW_MAKER:
        assert name in rows, sorted(rows)
        r = rows[name]
        assert (r["vspill"], r["sspill"], r["scratch"]) == (0, 0, 0), r


def test_pair_scatter_keeps_two_workgroups_per_cu(sort_rows):
    for b in (8, 9):
        pairs, keys = sort_rows["k_radix_scatter_pairs<%d>" % b], sort_rows["k_radix_scatter<%d>" % b]
        assert pairs["lds"] == keys["lds"]  # the values take the words' 64 KB, after them
        assert pairs["vgpr"] <= 128 and pairs["occ"] == keys["occ"] == 4


def test_existing_sort_and_maker_kernels_keep_their_resources(K, sort_rows):
    assert {n: (r["vgpr"], r["lds"], r["occ"]) for n, r in sort_rows.items() if n not in NEW} == SORT_BEFORE
    maker = K.table("gt4hip_maker.hip")
    assert {r["name"]: (r["vgpr"], r["lds"], r["occ"]) for r in maker} == {**MAKER_BEFORE, **MAKER_NEW}
