"""The kernels of gt4hip_subset.hip exist and neither spill nor touch scratch memory (tools/kernel_resources.py; hipcc
cross-compiles gfx950 without a GPU)."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def rows():
    if not shutil.which("hipcc"):
        pytest.skip("hipcc not on PATH")
    import kernel_resources
    return kernel_resources.table("gt4hip_subset.hip")


def test_subset_kernels_exist(rows):
    names = {r["name"] for r in rows}
    # <weighted ratio, what the pass writes: 0 nothing, 1 records, 2 occurrences per record>
    for want in ("k_subset_pass<false, 0>", "k_subset_pass<true, 0>", "k_subset_pass<false, 1>", "k_subset_pass<true, 1>", "k_subset_pass<false, 2>",
                 "k_subset_scan_reduce<0>", "k_subset_scan_apply<0>", "k_subset_scan_reduce<1>", "k_subset_scan_apply<1>", "k_subset_scan_reduce<2>",
                 "k_subset_scan_apply<2>", "k_subset_guess", "k_subset_changed", "k_subset_compact"):
        assert want in names, (want, sorted(names))


def test_subset_kernels_do_not_spill(rows):
    bad = [(r["name"], r["vspill"], r["sspill"], r["scratch"]) for r in rows if r["vspill"] or r["sspill"] or r["scratch"]]
    assert not bad, bad
    assert all(0 <= r["lds"] <= 64 << 10 for r in rows), rows  # the weighted pass stages a tile's inputs: 12 bytes per item
