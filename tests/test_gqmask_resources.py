"""The masking kernels (gt4hip_mask.hip) exist in all their instantiations, may not spill or touch scratch memory, the probing
one keeps the 64 VGPRs the query family holds (eight wavefronts per SIMD hide the probe's dependent loads) and their LDS
leaves room for the workgroups a CU runs side by side (tools/kernel_resources.py; hipcc cross-compiles gfx950 without a GPU)."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

LDS_PER_CU = 160 * 1024  # gfx950
KERNELS = ("k_mask_ends<true>", "k_mask_ends<false>", "k_mask_apply<true>", "k_mask_apply<false>")


@pytest.fixture(scope="module")
def rows():
    if not shutil.which("hipcc"):
        pytest.skip("hipcc not on PATH")
    import kernel_resources
    return {r["name"]: r for r in kernel_resources.table("gt4hip_mask.hip")}


def test_every_instantiation_is_there(rows):
    for want in KERNELS:
        assert want in rows, sorted(rows)


def test_no_spills_no_scratch_and_the_query_family_s_registers(rows):
    bad = [(n, r["vspill"], r["sspill"], r["scratch"]) for n, r in rows.items() if r["vspill"] or r["sspill"] or r["scratch"]]
    assert not bad, bad
    assert rows["k_mask_ends<true>"]["vgpr"] <= 64 and rows["k_mask_ends<false>"]["vgpr"] <= 64, rows
    # the streaming pass over the text holds a thread's 16 bytes and little else
    assert rows["k_mask_apply<true>"]["vgpr"] <= 64 and rows["k_mask_apply<false>"]["vgpr"] <= 64, rows


def test_two_workgroups_and_more_share_a_cu_s_lds(rows):
    for name in KERNELS:
        assert 2 * rows[name]["lds"] <= LDS_PER_CU, rows[name]
        assert rows[name]["lds"] <= 64, rows[name]  # the block scan's wavefront sums alone
