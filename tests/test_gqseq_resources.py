"""The per-sequence profile kernels (gt4hip_seqprofile.hip) may not spill or touch scratch memory, keep the 64 VGPRs the
query family holds (eight wavefronts per SIMD hide the probe's dependent loads) and leave LDS for the workgroups a CU runs
side by side (tools/kernel_resources.py; hipcc cross-compiles gfx950 without a GPU)."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

LDS_PER_CU = 160 * 1024  # gfx950


@pytest.fixture(scope="module")
def rows():
    if not shutil.which("hipcc"):
        pytest.skip("hipcc not on PATH")
    import kernel_resources
    return kernel_resources.table("gt4hip_seqprofile.hip")


def test_both_instantiations_and_the_zeroing_kernel_are_there(rows):
    names = [r["name"] for r in rows]
    for want in ("k_seq_profile<true>", "k_seq_profile<false>", "k_seq_zero"):
        assert want in names, names


def test_no_spills_no_scratch_and_the_query_family_s_registers(rows):
    bad = [(r["name"], r["vspill"], r["sspill"], r["scratch"]) for r in rows if r["vspill"] or r["sspill"] or r["scratch"]]
    assert not bad, bad
    assert all(r["vgpr"] <= 64 for r in rows), rows


def test_two_workgroups_and_more_share_a_cu_s_lds(rows):
    for r in rows:
        if r["name"].startswith("k_seq_"):
            assert 2 * r["lds"] <= LDS_PER_CU, r
    # the boundary runs of a tile: 64 entries of (sequence, sum, words, hits)
    prof = {r["name"]: r["lds"] for r in rows}
    assert prof["k_seq_profile<true>"] <= 64 * 24 and prof["k_seq_profile<false>"] <= 64 * 24, prof
