"""glistcompare -mm N without a GPU: what the CLI decides before any device work, the exported entry point, the
kernels' resources, and the numpy model of the rules (tests/mismatch_model.py) on hand-made cases."""
import ctypes
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import mismatch_model as MM
import mismatch_util as MU
from genometester4_amd.listio import make_records, write_list

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "genometester4_amd", "glistcompare")
GOLDEN = os.path.join(ROOT, "tests", "golden", "mm_cases.json")


@pytest.fixture(scope="module")
def lists():
    d = tempfile.mkdtemp(prefix="gt4mm_cpu_")
    a, b = MU.dense_pair(3, 4)
    for name, rec in (("a", a), ("b", b), ("c", a)):
        write_list(os.path.join(d, name + ".list"), rec, 4)
    yield d
    import shutil
    shutil.rmtree(d, ignore_errors=True)


def _run(argv, cwd, env=None):
    e = dict(os.environ)
    e.update(env or {})
    before = set(os.listdir(cwd))
    r = subprocess.run([CLI] + argv, cwd=cwd, capture_output=True, env=e, timeout=120)
    made = sorted(set(os.listdir(cwd)) - before)
    for f in made:
        os.unlink(os.path.join(cwd, f))
    return r, made


def _device_count():
    from genometester4_amd import capi
    return capi.lib().gt4hip_device_count()


def test_union_with_mismatches_warns_and_writes_nothing(lists):
    r, made = _run(["a.list", "b.list", "-u", "-mm", "1"], lists)
    assert r.returncode == 0, r.stderr
    assert r.stderr.decode() == "Warning: Number of mismatches are not used!\n"
    assert r.stdout == b"" and made == []


def test_intersection_with_mismatches_writes_nothing_and_debug_lines(lists):
    r, made = _run(["a.list", "b.list", "-i", "-mm", "2", "-D"], lists)
    assert r.returncode == 0 and made == []
    err = r.stderr.decode()
    assert "Warning: Number of mismatches are not used!\n" in err
    assert "compare_wordmaps; List 2: " in err and "Table 2: " in err
    assert "Finding diff" not in err


def test_three_files_keep_the_mismatch_error(lists):
    r, made = _run(["a.list", "b.list", "c.list", "-u", "-mm", "1"], lists)
    assert r.returncode == 1 and made == []
    assert r.stderr.decode().startswith("Error: Multiple files are not compatible with mismatches!\n")


def test_several_gpus_are_refused(lists):
    r, made = _run(["a.list", "b.list", "-d", "-mm", "1", "--gpus", "2"], lists)
    assert r.returncode == 1 and made == []
    assert "-mm needs both lists resident on one GPU" in r.stderr.decode()
    r, made = _run(["a.list", "b.list", "-dd", "-mm", "1"], lists, env={"GT4HIP_HBM_LIMIT": "1G"})
    assert r.returncode == 1 and made == []
    assert "GT4HIP_HBM_LIMIT" in r.stderr.decode()


def test_difference_without_a_device_fails_loudly(lists):
    r, made = _run(["a.list", "b.list", "-d", "-mm", "1"], lists)
    if _device_count() == 0:
        assert r.returncode == 1 and made == []
        assert r.stderr.decode().startswith("Error: ")
    else:
        assert r.returncode == 0 and made == ["out_4_1_diff1.list"]


def test_entry_points_are_exported():
    from genometester4_amd import capi
    L = ctypes.CDLL(capi.LIB_PATH)
    assert hasattr(L, "gt4hip_compare_mismatch") and hasattr(L, "gt4hip_mismatch_stats_get")
    assert "gt4hip_compare_mismatch" in capi.SYMBOLS


def test_mismatch_kernels_do_not_spill():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    rows = kernel_resources.table("gt4hip_mismatch.hip")
    assert {r["name"].split("<")[0] for r in rows} >= {"k_index_build", "k_prepass", "k_level", "k_decide", "k_scatter"}
    for r in rows:
        assert r["vspill"] == 0 and r["sspill"] == 0 and r["scratch"] == 0, r


def test_golden_no_device_cases_replay(lists):
    """the golden cases that never reach a device: -u / -i with -mm, replayed byte for byte"""
    with open(GOLDEN) as f:
        g = json.load(f)
    cases = [c for c in g["cases"] if not any(op in c["argv"] for op in ("-d", "-dd", "-du"))]
    assert len(cases) >= 4
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_mm as MG
    d = tempfile.mkdtemp(prefix="gt4mm_nodev_")
    files = MG.build_inputs(sorted({c["input"] for c in cases}), d)
    run = os.path.join(d, "run")
    os.mkdir(run)
    for c in cases:
        argv = ["../" + a if a in files.values() else a for a in c["argv"]]
        r, made = _run(argv, run)
        assert (r.returncode, r.stdout.decode(), r.stderr.decode(), made) == (c["exit"], c["stdout"], c["stderr"], sorted(c["files"])), c["id"]


def test_model_variant_counts_and_revcomp():
    assert len(MM.variant_masks(25, 1)) == 75 and len(MM.variant_masks(25, 3)) == 62100
    assert len(MM.variant_masks(4, 5)) == 0
    m = MM.variant_masks(32, 1)
    assert int(m.max()) == 3 << 62
    w = np.array([0, (1 << 64) - 1, 0x1B], dtype=np.uint64)
    assert [int(x) for x in MU.revcomp(w, 32)] == [(1 << 64) - 1, 0, int(MU.revcomp(np.array([0x1B], dtype=np.uint64), 32)[0])]
    # ACGT (0,1,2,3 from the first base in the high bits) is its own reverse complement
    acgt = np.array([0b00011011], dtype=np.uint64)
    assert int(MU.revcomp(acgt, 4)[0]) == 0b00011011


def test_model_counts_presence_not_counts():
    # A = {AAAA}; B holds AAAC (one mismatch) with a large count: s = 1 (present), not 99
    a = make_records(np.array([0], dtype=np.uint64), np.array([5], dtype=np.uint32))
    b = make_records(np.array([1], dtype=np.uint64), np.array([99], dtype=np.uint32))
    assert len(MM.compare_mismatch(a, b, 4, 1, cutoff=2)[4]) == 1
    assert len(MM.compare_mismatch(a, b, 4, 1, cutoff=1)[4]) == 0
