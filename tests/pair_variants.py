"""Which k_pair_merge<NT, IPT, MODE, OPS, FAST, OPSET> instantiation a call launches: a Python restatement of the host's
selection, and the matrix of calls tests/test_pair_variants.py runs so that every launchable instantiation is reached.

The restated C++ (genometester4_amd/csrc), by file: function:
  gt4hip_pair.hip     gt4hip_compare (per-stream default rules), gt4hip_run_pair (ops 8 -> 4 on (B, A), shorter list
                      first for an intersection, geometry, "dynamic", "scan_group", the two-pass path)
  gt4hip_multi.hip    gt4hip_nway_params, gt4hip_union_multi (the pairwise tree), gt4hip_intersect_multi (the chain)
  gt4hip_table.hip    table_column_by_union, gt4hip_probe_table_ex
  gt4hip_pair_variant.h  merge_ipt, pair_variant (the class of p.ops, FAST, OPSET), merge_tile_records
tests/test_pair_variant_map.py ties this map to the instantiations the compiler emits and to pair_variant itself.
No GPU and no library are needed to import this module."""
from __future__ import annotations

from collections import namedtuple

MODE_COUNT, MODE_LOOKBACK, MODE_OFFSETS = 0, 1, 2        # gt4hip_pair_variant.h: enum MergeMode
FILTER_REFERENCE, FILTER_RAW, FILTER_RESULT = 0, 1, 2    # gt4hip_pair_variant.h: enum Filter
RULE_DEFAULT, RULE_ADD, RULE_SUBTRACT, RULE_MIN, RULE_MAX, RULE_FIRST, RULE_SECOND, RULE_NUMBER = range(8)
RULE_MINZ = 8                                            # gt4hip_pair_variant.h: RULE_MINZ
OP_UNION, OP_INTRSEC, OP_DIFF1, OP_DIFF2 = 1, 2, 4, 8

GT4_IPT_UNION, GT4_IPT_INTERSECT, GT4_IPT_INTERSECT_SMALL, MERGE_VT = 4, 6, 4, 4   # gt4hip_pair_variant.h: GT4_IPT_*, MERGE_VT
MERGE_TILE_SLACK = 64                                                             # gt4hip_pair_variant.h: MERGE_TILE_SLACK

# PairParams, reduced to what the selection reads
Params = namedtuple("Params", "ops rule cutoff subtract filter")


def compare_params(ops, rule=RULE_DEFAULT, cutoff=1, subtract=0):
    """gt4hip_pair.hip: gt4hip_compare: DEFAULT resolves per stream to ADD / MIN / SUBTRACT / SUBTRACT"""
    r = rule
    return Params(ops, (r or RULE_ADD, r or RULE_MIN, r or RULE_SUBTRACT, r or RULE_SUBTRACT), cutoff, 1 if subtract else 0,
                  FILTER_REFERENCE)


def nway_params(op_bit, rule, cutoff, filt):
    """gt4hip_multi.hip: gt4hip_nway_params: one rule for every stream, no -du"""
    return Params(op_bit, (rule,) * 4, cutoff, 0, filt)


def ops_class(ops):
    """gt4hip_pair_variant.h: pair_variant, cls"""
    return ops if ops in (1, 2, 4) else 0


def merge_ipt(nt, cls):
    """gt4hip_pair_variant.h: merge_ipt"""
    if nt == 1024 and cls == 2:
        return GT4_IPT_INTERSECT
    if nt == 1024 and cls == 1:
        return GT4_IPT_UNION
    if nt == 512 and cls == 2:
        return GT4_IPT_INTERSECT_SMALL
    return MERGE_VT


def merge_tile_records(geom, ops):
    """gt4hip_pair_variant.h: merge_tile_records of pair_variant (geom, any mode, p)"""
    nt = 1024 if geom else 512
    return nt * merge_ipt(nt, ops_class(ops)) - MERGE_TILE_SLACK


def fast_variant(cls, p):
    """gt4hip_pair_variant.h: pair_variant, fast"""
    fast = 0
    if p.filter == FILTER_REFERENCE:
        if cls == 1 and p.rule[0] == RULE_ADD:
            fast = 1
        if cls == 2 and p.rule[1] == RULE_MIN:
            fast = 1
        if cls == 4 and p.rule[2] == RULE_SUBTRACT and not p.subtract:
            fast = 1
    elif cls == 1 and p.rule[0] == RULE_ADD:
        fast = 2 if p.filter == FILTER_RAW else 3
    elif cls == 2 and p.rule[1] == RULE_MINZ:
        fast = 2 if p.filter == FILTER_RAW else 3
    if (cls == 0 and p.filter == FILTER_REFERENCE and not p.subtract and (not p.ops & 1 or p.rule[0] == RULE_ADD)
            and (not p.ops & 2 or p.rule[1] == RULE_MIN) and (not p.ops & 4 or p.rule[2] == RULE_SUBTRACT)
            and (not p.ops & 8 or p.rule[3] == RULE_SUBTRACT)):
        fast = 1
    return fast


def kernel_name(nt, mode, p):
    """gt4hip_pair_variant.h: pair_variant, as the compiler prints the instantiation"""
    cls = ops_class(p.ops)
    fast = fast_variant(cls, p)
    ipt = merge_ipt(nt, cls)
    # the fixed output sets: any-combination kernel, FAST 1, ops 3 / 5 / 15, and (512, COUNT) or (1024, not COUNT)
    if cls == 0 and fast == 1 and p.ops in (3, 5, 15) and (nt == 512 if mode == MODE_COUNT else nt == 1024):
        return "k_pair_merge<%d, %d, %d, 0, 1, %d>" % (nt, ipt, mode, p.ops)
    # F2 / F3 exist for the union and the intersection only; any other FAST falls back to 0
    if fast in (2, 3) and cls not in (1, 2):
        fast = 0
    return "k_pair_merge<%d, %d, %d, %d, %d, 0>" % (nt, ipt, mode, cls, fast)


Launch = namedtuple("Launch", "names swapped tiles")


def run_pair(p, nA, nB, count_only=False, two_pass=False, geom=None):
    """gt4hip_pair.hip: gt4hip_run_pair: the names launched (one, or two on the two-pass path), whether (A, B) went in
    swapped, and the number of merge tiles.  geom: None (automatic), 0 or 1 (options "geom0" / "geom1")."""
    swapped = False
    if p.ops == 8:  # the second complement alone is the first complement of (B, A)
        rule = list(p.rule)
        rule[2] = p.rule[3]
        p = p._replace(ops=4, rule=tuple(rule), subtract=0)
        nA, nB, swapped = nB, nA, True
    if p.ops == 2 and nA > nB and p.rule[1] not in (RULE_SUBTRACT, RULE_MINZ):  # shorter list first
        rule = list(p.rule)
        rule[1] = {RULE_FIRST: RULE_SECOND, RULE_SECOND: RULE_FIRST}.get(rule[1], rule[1])
        p = p._replace(rule=tuple(rule))
        nA, nB, swapped = nB, nA, not swapped
    if not nA + nB or not p.ops:
        return Launch([], swapped, 0)
    g = (0 if count_only else 1) if geom is None else geom                        # geometry
    tr = merge_tile_records(g, p.ops)
    tiles = (nA + nB + tr - 1) // tr
    nt = 1024 if g else 512
    if count_only:
        names = [kernel_name(nt, MODE_COUNT, p)]
    elif two_pass:                                                                 # count, scan, write
        names = [kernel_name(nt, MODE_COUNT, p), kernel_name(nt, MODE_OFFSETS, p)]
    else:
        names = [kernel_name(nt, MODE_LOOKBACK, p)]
    return Launch(names, swapped, tiles)


def compare_launches(ops, rule=0, cutoff=1, subtract=0, nA=1, nB=1, **path):
    return run_pair(compare_params(ops, rule, cutoff, subtract), nA, nB, **path)


def union_multi_steps(sizes, rule=RULE_DEFAULT, cutoff=1):
    """gt4hip_union_multi by the pairwise tree (option "kway" = 0, or fewer than three non-empty lists):
    [(Params, nA, nB, final)]; the inner levels run FILTER_RAW, the last merge (nway_final) FILTER_RESULT.
    Sizes of intermediate results are upper bounds (the union's size is at most the sum)."""
    rule = RULE_ADD if rule == RULE_DEFAULT else rule                              # DEFAULT resolves to ADD
    work = [n for n in sizes if n]                                                 # empty lists dropped
    steps = []
    if not work:
        return steps
    while len(work) > 2:                                                           # the pairwise tree
        nxt = []
        for i in range(0, len(work) - 1, 2):
            steps.append((nway_params(OP_UNION, rule, cutoff, FILTER_RAW), work[i], work[i + 1], False))
            nxt.append(work[i] + work[i + 1])
        if len(work) & 1:
            nxt.append(work[-1])
        work = nxt
    steps.append((nway_params(OP_UNION, rule, cutoff, FILTER_RESULT), work[0], work[1] if len(work) > 1 else 0, True))
    return steps


def intersect_multi_steps(sizes, rule=RULE_DEFAULT, cutoff=1):
    """gt4hip_intersect_multi: the left-to-right chain, MIN as RULE_MINZ, inner steps FILTER_RAW,
    the last FILTER_RESULT; one list: a union with an empty list under FIRST / NUMBER."""
    rule = RULE_MIN if rule == RULE_DEFAULT else rule                              # DEFAULT resolves to MIN
    if not sizes or any(n == 0 for n in sizes):                                    # an empty list: empty_result
        return []
    krule = RULE_MINZ if rule == RULE_MIN else rule
    if len(sizes) == 1:
        r = RULE_NUMBER if rule == RULE_NUMBER else RULE_FIRST
        return [(nway_params(OP_UNION, r, cutoff, FILTER_RESULT), sizes[0], 0, True)]
    steps = []
    acc = sizes[0]
    for k in range(1, len(sizes) - 1):
        steps.append((nway_params(OP_INTRSEC, krule, cutoff, FILTER_RAW), acc, sizes[k], False))
        acc = min(acc, sizes[k])
    steps.append((nway_params(OP_INTRSEC, krule, cutoff, FILTER_RESULT), acc, sizes[-1], True))
    return steps


def union_table_steps(n_keys, sizes, presence=False):
    """The count tables by merges (option "kway" = 0): gt4hip_probe_table_ex intersects the base with every list under
    SECOND (NUMBER for presence), FILTER_RAW, then table_column_by_union takes union (keys, L_j) under SECOND,
    FILTER_RAW."""
    steps = []
    for n in sizes:
        steps.append((nway_params(OP_INTRSEC, RULE_NUMBER if presence else RULE_SECOND, 0, FILTER_RAW), n_keys, n, False))
        steps.append((nway_params(OP_UNION, RULE_SECOND, 0, FILTER_RAW), n_keys, n, False))
    return steps


def multi_launches(steps, count_only=False, two_pass=False, geom=None):
    """names of every step of an N-way call: inner levels always write records, only the last may count"""
    names = []
    for p, na, nb, final in steps:
        names += run_pair(p, na, nb, count_only=count_only and final, two_pass=two_pass, geom=geom).names
    return names


# ---------------------------------------------------------------- the GPU matrix (tests/test_pair_variants.py)

U32 = 0xFFFFFFFF
CUTOFFS = (0, 1, 3, U32)

# paths: (id, options set on the context, count_only); geometry / two-pass as run_pair reads them
PATHS = (
    ("default", {}, False),
    ("count_only", {}, True),
    ("two_pass", {"two_pass": 1}, False),
    ("geom0", {"geom0": 1}, False),
    ("geom0_two_pass", {"geom0": 1, "two_pass": 1}, False),
    ("geom1_count_only", {"geom1": 1}, True),
    ("scan_group1", {"scan_group": 1}, False),
    ("scan_group-1", {"scan_group": -1}, False),
    ("dynamic", {"dynamic": None}, False),       # None: 1 for ops 4 / 8 (round-robin by default), -1 for the others
)
RESET = {"two_pass": 0, "geom0": 0, "scan_group": 0, "dynamic": 0, "kway": 1}


def path_options(path, ops):
    pid, opts, count_only = next(x for x in PATHS if x[0] == path)
    opts = dict(opts)
    if "dynamic" in opts:
        opts["dynamic"] = 1 if ops in (4, 8) else -1
    return opts, count_only


def path_geometry(path):
    """(count_only, two_pass, geom) of a path, as run_pair sees them"""
    opts, count_only = path_options(path, 0)
    geom = 0 if opts.get("geom0") else (1 if opts.get("geom1") else None)
    return count_only, bool(opts.get("two_pass")), geom


# (ops, rule, cutoff, subtract): every call of the main input, each under every path
PAIR_CALLS = (
    [(ops, 0, c, 0) for ops, c in ((1, 1), (2, 3), (4, 0), (8, U32))]                      # FAST 1, single outputs
    + [(ops, r, c, 0) for ops in (1, 2, 4, 8) for r, c in ((RULE_MAX, 3), (RULE_SECOND, 1), (RULE_SUBTRACT, 0))]  # FAST 0
    + [(1, RULE_ADD, U32, 0), (2, RULE_MIN, 0, 0), (2, RULE_FIRST, U32, 0), (4, RULE_NUMBER, 3, 0)]
    + [(4, 0, 1, 1), (15, 0, 3, 1), (5, RULE_ADD, 0, 1)]                                   # -du
    + [(ops, 0, c, 0) for ops, c in ((3, 1), (5, 3), (15, 0), (15, U32))]                  # OPSET
    + [(ops, 0, c, 0) for ops, c in ((6, 1), (7, 3), (9, 0), (10, U32), (12, 1), (14, 3))]  # FAST 1, OPSET 0
    + [(15, r, c, 0) for r, c in ((RULE_ADD, 1), (RULE_MAX, 3), (RULE_MIN, 0), (RULE_FIRST, U32), (RULE_NUMBER, 1))]  # FAST 0
)
# (entry, number of lists, rule, cutoff): the N-way calls over the main input's lists, union_multi with "kway" = 0
MULTI_CALLS = (
    ("union_multi", 3, RULE_DEFAULT, 3), ("union_multi", 5, RULE_DEFAULT, U32), ("union_multi", 4, RULE_MAX, 1),
    ("intersect_multi", 3, RULE_DEFAULT, 1), ("intersect_multi", 4, RULE_DEFAULT, 3), ("intersect_multi", 5, RULE_ADD, 0),
)
# the other inputs: a cross-section of classes under the default and the two-pass path
SIDE_CALLS = ((15, 0, 1, 0), (1, 0, 3, 0), (2, 0, 1, 0), (2, RULE_FIRST, 0, 0), (8, 0, 1, 0), (6, RULE_MAX, 1, 0))
SIDE_PATHS = ("default", "two_pass", "count_only")


def multi_steps(entry, sizes, rule, cutoff):
    return (union_multi_steps if entry == "union_multi" else intersect_multi_steps)(sizes, rule, cutoff)


def predicted(call, path, sizes):
    """names a matrix case launches: call = ("pair", ops, rule, cutoff, subtract) or (entry, n, rule, cutoff)"""
    count_only, two_pass, geom = path_geometry(path)
    if call[0] == "pair":
        _, ops, rule, cutoff, sub = call
        return compare_launches(ops, rule, cutoff, sub, sizes[0], sizes[1], count_only=count_only, two_pass=two_pass,
                                geom=geom).names
    entry, n, rule, cutoff = call
    return multi_launches(multi_steps(entry, list(sizes[:n]), rule, cutoff), count_only, two_pass, geom)


def matrix():
    """every (call, path) of the main input"""
    cases = [(("pair",) + c, path) for c in PAIR_CALLS for path, _, _ in PATHS]
    cases += [(c, path) for c in MULTI_CALLS for path, _, _ in PATHS]
    return cases


def launchable_from_matrix(main_sizes=(3_300_000,) * 5):
    names = set()
    for call, path in matrix():
        names.update(predicted(call, path, main_sizes))
    return names
