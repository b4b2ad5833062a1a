"""The variant map of tests/pair_variants.py against the product, without a GPU: every compiled k_pair_merge<...>
instantiation is reached by a case of the GPU matrix (tests/test_pair_variants.py), and for every call the map is asked
about, the product's own selection (gt4hip_pair_variant.h, compiled here into tests/harness/pair_variant_print.cc) names
the same instantiation and the same tile length.  Adding an instantiation, or changing the selection so that a variant
drops out of the matrix or the map no longer follows it, fails here first (hipcc cross-compiles gfx950 without a GPU)."""
import os
import shutil
import subprocess
import sys

import pytest

import pair_variants as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

MAIN = (3_300_000,) * 5   # sizes of the GPU matrix's main lists (test_pair_variants.py asserts its inputs against the map's tiles)


@pytest.fixture(scope="module")
def compiled():
    if not shutil.which("hipcc"):
        pytest.skip("hipcc not on PATH")
    import kernel_resources as K
    names = {r["name"] for r in K.table("gt4hip_kernels.hip") if r["name"].startswith("k_pair_merge<")}
    assert names, "no k_pair_merge instantiation in the resource table"
    return names


def _predicted():
    names = set()
    for call, path in V.matrix():
        names.update(V.predicted(call, path, MAIN))
    return names


def test_every_compiled_instantiation_is_reached(compiled):
    missing = sorted(compiled - _predicted())
    assert not missing, "compiled and not reached by the GPU matrix: %s" % missing


def test_matrix_predicts_only_compiled_names(compiled):
    side = set()
    for c in V.SIDE_CALLS:
        for path in V.SIDE_PATHS:
            side.update(V.predicted(("pair",) + c, path, (3_000_000, 300_000)))
            side.update(V.predicted(("pair",) + c, path, (300_000, 3_000_000)))
    extra = sorted((_predicted() | side) - compiled)
    assert not extra, "the map predicts instantiations that are not compiled: %s" % extra


def test_map_restates_the_argument_swaps():
    # ops 8 alone: the first complement of (B, A), on the class-4 kernel
    l8 = V.compare_launches(8, nA=10, nB=20)
    assert l8.swapped and l8.names == ["k_pair_merge<1024, 4, 1, 4, 1, 0>"]
    # an intersection puts the shorter list first, except under SUBTRACT (asymmetric); FIRST becomes SECOND
    assert V.compare_launches(2, V.RULE_FIRST, nA=20, nB=10).swapped
    assert not V.compare_launches(2, V.RULE_FIRST, nA=10, nB=20).swapped
    assert not V.compare_launches(2, V.RULE_SUBTRACT, nA=20, nB=10).swapped
    # ... and never the N-way chain's running MIN
    p = V.nway_params(V.OP_INTRSEC, V.RULE_MINZ, 1, V.FILTER_RAW)
    assert not V.run_pair(p, 20, 10).swapped
    # -du takes the general kernel of the first complement (FAST 0), without -du the folded one
    assert V.compare_launches(4, subtract=1, nA=1, nB=1).names == ["k_pair_merge<1024, 4, 1, 4, 0, 0>"]
    # the second complement's own rule goes to the swapped call: -r max (FAST 0), default (FAST 1)
    assert V.compare_launches(8, V.RULE_MAX, count_only=True).names == ["k_pair_merge<512, 4, 0, 4, 0, 0>"]


def test_map_names_the_nway_filters():
    # union_multi, pairwise tree: RAW (FAST 2) at the inner levels, RESULT (FAST 3) at the last
    steps = V.union_multi_steps([5, 6, 7])
    assert [s[0].filter for s in steps] == [V.FILTER_RAW, V.FILTER_RESULT]
    assert V.multi_launches(steps) == ["k_pair_merge<1024, 4, 1, 1, 2, 0>", "k_pair_merge<1024, 4, 1, 1, 3, 0>"]
    # intersect_multi: MIN runs as RULE_MINZ, FAST 2 then 3; a count-only call counts its last step only
    steps = V.intersect_multi_steps([5, 6, 7, 8])
    assert [s[0].rule[1] for s in steps] == [V.RULE_MINZ] * 3
    assert V.multi_launches(steps, count_only=True) == ["k_pair_merge<1024, 6, 1, 2, 2, 0>"] * 2 + ["k_pair_merge<512, 4, 0, 2, 3, 0>"]
    # the count tables: SECOND / NUMBER under RAW, the general kernels (FAST 0)
    names = V.multi_launches(V.union_table_steps(9, [4, 5], presence=True))
    assert set(names) == {"k_pair_merge<1024, 6, 1, 2, 0, 0>", "k_pair_merge<1024, 4, 1, 1, 0, 0>"}


@pytest.fixture(scope="module")
def selection(tmp_path_factory):
    """the product's selection as a function of [(nt, mode, Params)]: [(name, records per tile)]"""
    exe = str(tmp_path_factory.mktemp("pair_variant") / "pair_variant_print")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "genometester4_amd", "csrc"),
                    os.path.join(ROOT, "tests", "harness", "pair_variant_print.cc"), "-o", exe], check=True)

    def ask(cases):
        text = "".join("%d %d %d %d %d %d %d %d %d %d\n" % ((nt == 1024, mode, p.ops) + tuple(p.rule) + (p.cutoff, p.subtract, p.filter))
                       for nt, mode, p in cases)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(cases)
        return [(ln.rsplit(" ", 1)[0], int(ln.rsplit(" ", 1)[1])) for ln in out]
    return ask


def test_map_agrees_with_the_compiled_selection(selection, monkeypatch):
    asked = []
    kernel_name = V.kernel_name
    monkeypatch.setattr(V, "kernel_name", lambda nt, mode, p: asked.append((nt, mode, p)) or kernel_name(nt, mode, p))
    _predicted()                                                                   # V.matrix()
    for c in V.SIDE_CALLS:
        for path in V.SIDE_PATHS:
            V.predicted(("pair",) + c, path, (3_000_000, 300_000))
            V.predicted(("pair",) + c, path, (300_000, 3_000_000))
    for presence in (False, True):
        for path in ({}, {"two_pass": True}, {"geom": 0}):
            V.multi_launches(V.union_table_steps(9, [4, 5], presence=presence), **path)
    test_map_restates_the_argument_swaps()
    test_map_names_the_nway_filters()
    cases = sorted(set(asked))
    assert len(cases) > 100
    expected = [(kernel_name(nt, mode, p), V.merge_tile_records(nt == 1024, p.ops)) for nt, mode, p in cases]
    wrong = [(c, got, exp) for c, got, exp in zip(cases, selection(cases), expected) if got != exp]
    assert not wrong, "(nt, mode, Params), the product's selection, the map's: %s" % wrong[:5]
