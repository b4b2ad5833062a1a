"""The kernels of glistcompare --pairwise (gt4hip_pairwise.hip: the partial matrices for every lane-group width, one block of
list columns against itself and against another, and the reduction of the partials) may not spill or touch scratch memory
(tools/kernel_resources.py; hipcc cross-compiles gfx950 without a GPU)."""
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


def test_pairwise_kernels_do_not_spill(K):
    rows = K.table("gt4hip_pairwise.hip")
    names = [r["name"] for r in rows]
    want = ["k_pairwise_reduce", "k_pairwise_partial<32, false>"] + ["k_pairwise_partial<%d, true>" % g for g in (2, 4, 8, 16, 32)]
    assert sorted(names) == sorted(want), names
    bad = [(r["name"], r["vspill"], r["sspill"], r["scratch"]) for r in rows if r["vspill"] or r["sspill"] or r["scratch"]]
    assert not bad, bad
    assert all(r["vgpr"] <= 64 for r in rows), rows  # eight wavefronts per SIMD, as the grids are sized for
    assert max(r["lds"] for r in rows) <= 16384, rows  # two 32 x 32 matrices of 64-bit accumulators
