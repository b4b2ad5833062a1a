"""The variant map of tests/pair_variants.py against what the compiler emits: every compiled k_pair_merge<...>
instantiation is either reached by a case of the GPU matrix (tests/test_pair_variants.py) or listed here as unreachable,
with the reason.  Adding an instantiation, or changing the selection so that a variant drops out of the matrix, fails
here first (hipcc cross-compiles gfx950 without a GPU)."""
import os
import shutil
import sys

import pytest

import pair_variants as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

_OPSET = "launch_pair_merge_ops (gt4hip_kernels.hip:1312) takes the fixed output set only at (512, COUNT) or (1024, not COUNT)"
UNREACHABLE = {
    "k_pair_merge<1024, 4, 0, 0, 1, 3>": "1024-thread COUNT: " + _OPSET,
    "k_pair_merge<1024, 4, 0, 0, 1, 5>": "1024-thread COUNT: " + _OPSET,
    "k_pair_merge<1024, 4, 0, 0, 1, 15>": "1024-thread COUNT: " + _OPSET,
    "k_pair_merge<512, 4, 1, 0, 1, 3>": "512-thread LOOKBACK: " + _OPSET,
    "k_pair_merge<512, 4, 1, 0, 1, 5>": "512-thread LOOKBACK: " + _OPSET,
    "k_pair_merge<512, 4, 1, 0, 1, 15>": "512-thread LOOKBACK: " + _OPSET,
    "k_pair_merge<512, 4, 2, 0, 1, 3>": "512-thread OFFSETS: " + _OPSET,
    "k_pair_merge<512, 4, 2, 0, 1, 5>": "512-thread OFFSETS: " + _OPSET,
    "k_pair_merge<512, 4, 2, 0, 1, 15>": "512-thread OFFSETS: " + _OPSET,
}

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


def test_every_compiled_instantiation_is_reached_or_listed(compiled):
    reached = _predicted()
    missing = sorted(compiled - reached - set(UNREACHABLE))
    assert not missing, "compiled, not reached by the GPU matrix and not on the unreachable list: %s" % missing
    both = sorted(reached & set(UNREACHABLE))
    assert not both, "listed as unreachable, yet the matrix launches them: %s" % both


def test_unreachable_list_holds_only_compiled_names(compiled):
    assert not sorted(set(UNREACHABLE) - compiled)


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
