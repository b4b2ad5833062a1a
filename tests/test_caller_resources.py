"""The kernels of gmer_caller (gt4hip_caller.hip: the training objective and the per-marker probabilities) may not spill or
touch scratch memory (tools/kernel_resources.py, with the switch csrc/Makefile gives this source; hipcc cross-compiles
gfx950 without a GPU)."""
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


def test_caller_kernels_do_not_spill(K):
    rows = K.table("gt4hip_caller.hip")
    names = [r["name"] for r in rows]
    for want in ("k_caller_mlogl", "k_caller_probs<true>", "k_caller_probs<false>"):
        assert want in names, names
    bad = [(r["name"], r["vspill"], r["sspill"], r["scratch"]) for r in rows if r["vspill"] or r["sspill"] or r["scratch"]]
    assert not bad, bad
    assert all(r["vgpr"] <= 128 for r in rows), rows  # four wavefronts per SIMD at least: lgamma, exp and log in double, one copy each


def test_the_tool_builds_the_source_as_the_makefile_does(K):
    mk = open(os.path.join(ROOT, "genometester4_amd", "csrc", "Makefile")).read()
    assert "gt4hip_caller.hip.o: HIPFLAGS += $(CALLER_LICM)" in mk
    flags = mk.split("CALLER_LICM := ")[1].split("\n")[0].split()
    assert flags == K.PER_SOURCE["gt4hip_caller.hip"]
