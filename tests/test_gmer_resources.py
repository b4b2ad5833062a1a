"""The kernels of gmer_counter (gt4hip_gmer.hip: the db, the counting kernel, the statistics pass over a reader call's arrays)
may not spill or touch scratch memory (tools/kernel_resources.py; hipcc cross-compiles gfx950 without a GPU)."""
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


def test_gmer_kernels_do_not_spill(K):
    rows = K.table("gt4hip_gmer.hip")
    names = [r["name"] for r in rows]
    for want in ("k_gmer_prepare", "k_gmer_pack", "k_gmer_count<true>", "k_gmer_count<false>", "k_index_build", "k_mk_text_counts<false>",
                 "k_mk_text_counts<true>"):
        assert want in names, names
    bad = [(r["name"], r["vspill"], r["sspill"], r["scratch"]) for r in rows if r["vspill"] or r["sspill"] or r["scratch"]]
    assert not bad, bad
    assert all(r["vgpr"] <= 64 for r in rows), rows  # eight wavefronts per SIMD, as the grids are sized for
