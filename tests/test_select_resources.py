"""The kernels of glistcompare -u --min_lists / --max_lists (gt4hip_select.hip: the decision per row for every lane-group
width, both folds and both load widths, the scan of the segments, the emit) may not spill or touch scratch memory (tools/kernel_resources.py;
hipcc cross-compiles gfx950 without a GPU)."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def K():
    if not shutil.which("hipcc"):
        pytest.skip("hipcc not on PATH")
    import kernel_resources
    return kernel_resources


def test_select_kernels_do_not_spill(K):
    rows = K.table("gt4hip_select.hip")
    names = [r["name"] for r in rows]
    want = ["k_select_scan", "k_select_emit"] + ["k_select_decide<%d, %s, %d>" % (g, m, v) for g in (2, 4, 8, 16, 32, 64) for m in ("true", "false") for v in (1, 4)]
    for w in want:
        assert w in names, names
    bad = [(r["name"], r["vspill"], r["sspill"], r["scratch"]) for r in rows if r["vspill"] or r["sspill"] or r["scratch"]]
    assert not bad, bad
    assert all(r["vgpr"] <= 64 for r in rows), rows  # eight wavefronts per SIMD, as the grids are sized for
