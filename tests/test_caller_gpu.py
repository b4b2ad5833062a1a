"""gt4hip_caller.hip through capi against tests/caller_model.py (held to the reference in tests/test_caller_model.py), and
genometester4_amd/gmer_caller against every transcript of tests/golden/caller_cases.json.

Bounds (caller_model.Model.likelihoods, tolerance, mlogl): a likelihood may be off by 16 x 2^-52 x the largest of 1,
|lgamma (k + r)|, |log k!|, |k log p| and |r log (1 - p)|, added over its two densities, relative to the model's value
(plus 4 x 2^-1074 where the product is not a normal number); a sum of logarithms by the sum of its markers' bounds (a marker's: the
largest among its 15 likelihoods').  The
factor 16 is an allowance for the device's lgamma and exp; the largest error / bound seen is printed and kept in
profiles/caller/README.md."""
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import caller_model as M
import caller_util as U
import gmer_util as GU

pytestmark = pytest.mark.gpu

CASES = U.load_cases()
COUNTS = (0, 1, 2, 15, 16, 17, 255, 16383, 16384, 16390, 40000)
PAIRS = [(a, b) for a in COUNTS for b in COUNTS]
SIZES = (1, 63, 64, 65, 255, 256, 257, 2 * 256 + 1)
PB = 0.3
MODELS = {
    "diploid_lambda30": (0.0547219, 4.2603e-05, 0.014934, 0.985023, 30.0, 65.48, -0.6792684),
    "haploid": (0.0547219, 4.2603e-05, 0.985023, 0.014934, 30.0, 65.48, -0.6792684),
    "p_lisa_negative": (0.05, 0.1, 0.3, 0.7, 30.0, 65.48, -0.6792684),
    "size_nonpositive_at_2_lambda": (0.0547219, 4.2603e-05, 0.014934, 0.985023, 30.0, 65.48, -1.2),
    "size_nonpositive_everywhere": (0.05, 4.2603e-05, 0.014934, 0.985023, 30.0, 0.01, -0.6792684),
    "lambda_zero": (0.0547219, 4.2603e-05, 0.014934, 0.985023, 0.0, 65.48, -0.6792684),
}
WORST = dict(ratio=0.0, where=None)


@pytest.fixture(scope="module")
def ctx():
    from genometester4_amd import capi
    c = capi.Context(0)
    yield c
    c.close()
    print("\nlargest likelihood error / bound: %.4f at %s" % (WORST["ratio"], WORST["where"]))


_REF = {}


def _ref(name):
    """the model's likelihoods and bounds of every pair of COUNTS under MODELS[name], once"""
    if name not in _REF:
        m = M.Model(*MODELS[name], PB)
        _REF[name] = (m, {p: m.likelihoods(*p) for p in PAIRS})
    return _REF[name]


def _capi_model(name):
    from genometester4_amd import capi
    return capi.CallerModel(*[M.F(v) for v in MODELS[name]], M.F(PB))


def test_model_sets_are_what_they_claim():
    assert [t is None for t in _ref("size_nonpositive_at_2_lambda")[0].terms] == [False, False, False, False, True]
    assert all(t is None for t in _ref("size_nonpositive_everywhere")[0].terms)
    assert [t is None for t in _ref("lambda_zero")[0].terms] == [False, True, True, True, True]
    p = MODELS["p_lisa_negative"]
    assert p[1] + p[2] + p[3] > 1 and _ref("p_lisa_negative")[0].prior[6:] == [0.0] * 9


@pytest.mark.parametrize("name", list(MODELS))
@pytest.mark.parametrize("size", SIZES)
def test_probabilities_against_the_model(ctx, name, size):
    pairs = [PAIRS[(7 * size + i) % len(PAIRS)] for i in range(size)] if size < len(PAIRS) else [PAIRS[i % len(PAIRS)] for i in range(size)]
    s = ctx.caller_set([p[0] for p in pairs], [p[1] for p in pairs])
    cm = _capi_model(name)
    best, a_best, a_sum, a_all = s.probabilities(cm, all15=True)
    best2, a_best2, a_sum2, none = s.probabilities(cm)
    s.free()
    assert none is None and best.tobytes() == best2.tobytes() and a_best.tobytes() == a_best2.tobytes() and a_sum.tobytes() == a_sum2.tobytes()
    check_probabilities(name, pairs, best, a_best, a_sum, a_all)


def check_probabilities(name, pairs, best, a_best, a_sum, a_all):
    """what gt4hip_caller_probabilities gave for `pairs` (of PAIRS) under MODELS[name], all 15 likelihoods included, against
    the model: every marker"""
    _, ref = _ref(name)
    for i, p in enumerate(pairs):
        a, rel = ref[p]
        tol = [M.tolerance(a[j], rel[j]) for j in range(M.N_GT)]
        for j in range(M.N_GT):
            got = float(a_all[i, j])
            if a[j] != a[j]:
                assert got != got, (name, p, j, got)
                continue
            err = abs(got - a[j])
            if err / tol[j] > WORST["ratio"]:
                WORST.update(ratio=err / tol[j], where=(name, p, M.GT[j]))
            assert err <= tol[j], (name, p, j, got, a[j], err / tol[j])
        b = int(best[i])
        assert b < M.N_GT
        if any(v != v for v in a):
            assert a_sum[i] != a_sum[i]
        else:
            assert abs(float(a_sum[i]) - M.call(a)[1]) <= sum(tol)
        # the device's own strict > scan, first of equals
        dev = [float(v) for v in a_all[i]]
        assert b == M.call(dev)[0] and (a_best[i] == dev[b] or dev[b] != dev[b])
        if not any(v != v for v in a):
            mb = M.call(a)[0]
            second = max(v for j, v in enumerate(a) if j != mb)
            if a[mb] - second > tol[mb] + max(tol):
                assert b == mb, (name, p, b, mb)


def test_a_marker_without_any_likelihood_sums_to_zero(ctx):
    """X:7 of the goldens' edge.txt: 17,000 against 3 at coverage 20.  Every density of 17,000 underflows to 0, so all 15
    likelihoods and their sum are 0 -- the "-nan" the program prints there is the host's 0 / 0 -- and the best index stays 0."""
    from genometester4_amd import capi
    v = (0.0547219, 4.2603e-05, 0.014934, 0.985023, 20.0, 65.48, -0.6792684)
    m = M.Model(*v, PB)
    pairs = [(17000, 3), (3, 17000), (17000, 17000), (15, 17)]
    s = ctx.caller_set([p[0] for p in pairs], [p[1] for p in pairs])
    best, a_best, a_sum, a_all = s.probabilities(capi.CallerModel(*[M.F(x) for x in v], M.F(PB)), all15=True)
    s.free()
    for i, p in enumerate(pairs):
        a, rel = m.likelihoods(*p)
        for j in range(M.N_GT):
            assert a[j] == a[j] and abs(float(a_all[i, j]) - a[j]) <= M.tolerance(a[j], rel[j]), (p, j)
        if i < 3:
            assert a == [0.0] * M.N_GT and not a_all[i].any() and best[i] == 0 and a_best[i] == 0 and a_sum[i] == 0
    assert best[3] == 4  # AB


def _training_pairs():
    text = U.markers(seed=21, n_auto=6400, coverage=30.0)
    pairs = [(int(f[2]), int(f[3])) for f in (l.split(b"\t") for l in text.split(b"\n") if l)]
    pairs[5], pairs[300], pairs[2001] = (16384, 3), (40000, 40000), (255, 16390)
    return pairs


@pytest.fixture(scope="module")
def training(ctx):
    pairs = _training_pairs()
    s = ctx.caller_set([p[0] for p in pairs], [p[1] for p in pairs])
    yield pairs, s
    s.free()


MLOGL_RANGES = [(0, 1), (0, 255), (0, 256), (0, 257), (0, 2000), (0, 2001), (0, 6300), (1, 256), (77, 2001), (100, 6300), (6399, 1), (300, 1)]


@pytest.mark.parametrize("first,n", MLOGL_RANGES)
def test_mlogl_against_the_model_and_bit_for_bit_repeatable(ctx, training, first, n):
    pairs, s = training
    m = _ref("diploid_lambda30")[0]
    cm = _capi_model("diploid_lambda30")
    want, bound = M.mlogl(m, pairs[first:first + n])
    got = s.mlogl(cm, first, n)
    again = s.mlogl(cm, first, n)
    assert struct.pack("d", got) == struct.pack("d", again)
    print("mlogl [%d, +%d): %.17g against %.17g, error %.3g of %.3g allowed" % (first, n, got, want, abs(got - want), bound))
    assert abs(got - want) <= bound, (got, want, bound)
    assert s.last_ms() > 0


def test_mlogl_clamps_a_vanishing_likelihood_and_sums_nothing_to_minus_zero(ctx, training):
    pairs, s = training
    assert pairs[300] == (40000, 40000)
    cm = _capi_model("diploid_lambda30")
    a, _ = _ref("diploid_lambda30")[1][(40000, 40000)]
    assert sum(a) < 1e-30
    assert abs(s.mlogl(cm, 300, 1) - -M.log(1e-30)) <= 4 * M.EPS * 70
    t = ctx.caller_set([40000] * 3, [40000] * 3)
    assert abs(t.mlogl(cm) - -3 * M.log(1e-30)) <= 3 * 4 * M.EPS * 70 + 3 * M.EPS * 210
    t.free()
    assert struct.pack("d", s.mlogl(cm, 10, 0)) == struct.pack("d", -0.0)
    # other models between two calls of one model do not change its sum
    before = s.mlogl(cm)
    s.mlogl(_capi_model("haploid"))
    assert struct.pack("d", s.mlogl(cm)) == struct.pack("d", before)


def _cycled(n):
    """n markers, the 121 PAIRS over and over: the model evaluates 121 markers, not n"""
    return [PAIRS[i % len(PAIRS)] for i in range(n)]


def _cycled_mlogl(name, n):
    """(sum, bound) of caller_model.mlogl over _cycled (n): math.fsum of a pair's value x the times it occurs, and the sum of
    the per-marker bounds the model defines, a pair's bound x the times it occurs"""
    m = _ref(name)[0]
    times = [n // len(PAIRS) + (j < n % len(PAIRS)) for j in range(len(PAIRS))]
    each = [M.mlogl(m, [p]) for p in PAIRS]
    return math.fsum(v * t for (v, _), t in zip(each, times)), math.fsum(b * t for (_, b), t in zip(each, times))


@pytest.mark.parametrize("which", ["tree_second_trip", "max_grid"])
def test_mlogl_above_256_workgroups_and_at_the_largest_grid(ctx, which):
    """k_caller_mlogl adds the workgroups' sums with a loop over the grid in steps of a workgroup's threads: 65,536 + 257
    markers are 258 workgroups, so that loop takes a second trip; 262,144 + 257 markers are more than the 1024 workgroups
    the grid has at most, so the marker loop does (some threads add two markers).  Bit for bit repeatable, within the
    summed bound of the model, and bitwise the same under "grid_cap" = 1: the grid is a function of n alone.

    Largest error over its bound seen on an MI355X: 1.3e-5 at both sizes (profiles/caller/README.md)."""
    threads, most = ctx.get_counter("caller_threads"), ctx.get_counter("caller_max_grid")
    n = {"tree_second_trip": threads * threads, "max_grid": threads * most}[which] + threads + 1
    assert n == {"tree_second_trip": 65_536 + 257, "max_grid": 262_144 + 257}[which]
    assert ((n + threads - 1) // threads > threads) and ((n + threads - 1) // threads > most) == (which == "max_grid")
    pairs = _cycled(n)
    s = ctx.caller_set([p[0] for p in pairs], [p[1] for p in pairs])
    cm = _capi_model("diploid_lambda30")
    want, bound = _cycled_mlogl("diploid_lambda30", n)
    got = s.mlogl(cm)
    again = s.mlogl(cm)
    cut = ctx.get_counter("grid_capped")
    ctx.set_option("grid_cap", 1)
    try:
        capped = s.mlogl(cm)
    finally:
        ctx.set_option("grid_cap", 0)
    s.free()
    print("mlogl of %d markers: %.17g against %.17g, error %.3g of %.3g allowed (%.4f)" % (n, got, want, abs(got - want), bound, abs(got - want) / bound))
    assert struct.pack("d", got) == struct.pack("d", again)
    assert struct.pack("d", got) == struct.pack("d", capped) and ctx.get_counter("grid_capped") == cut
    assert abs(got - want) <= bound, (got, want, bound)


@pytest.mark.parametrize("name", ["diploid_lambda30", "size_nonpositive_at_2_lambda"])
def test_probabilities_in_pieces(ctx, name):
    """option "caller_piece" = 300 on 3 x 300 + 1 markers: three full pieces and one marker, byte for byte what the call gives
    in one piece, with and without all 15 likelihoods, and every marker against the model"""
    pairs = _cycled(3 * 300 + 1)
    s = ctx.caller_set([p[0] for p in pairs], [p[1] for p in pairs])
    cm = _capi_model(name)
    whole = s.probabilities(cm, all15=True), s.probabilities(cm)
    ctx.set_option("caller_piece", 300)
    ctx.set_option("poison", 1)  # (the device block of the pieces is not to hold the results of the whole)
    try:
        pieced = s.probabilities(cm, all15=True), s.probabilities(cm)
    finally:
        ctx.set_option("caller_piece", 0)
        ctx.set_option("poison", 0)
    s.free()
    for a, b in zip(whole, pieced):
        assert b[3] is None or b[3].shape == (len(pairs), M.N_GT)
        assert [x is None or x.tobytes() for x in a] == [x is None or x.tobytes() for x in b]
    assert [x.tobytes() for x in pieced[0][:3]] == [x.tobytes() for x in pieced[1][:3]]
    check_probabilities(name, pairs, *pieced[0])


def test_ranges_outside_the_set_are_refused(ctx, training):
    from genometester4_amd import capi
    _, s = training
    cm = _capi_model("haploid")
    for first, n in ((6401, 0), (0, 6401), (6400, 1)):
        with pytest.raises(capi.Gt4HipError) as e:
            s.mlogl(cm, first, n)
        assert e.value.code == capi.EINVAL
        with pytest.raises(capi.Gt4HipError):
            s.probabilities(cm, first, n)


@pytest.fixture(scope="module")
def workdir():
    d = U.make_workdir(CASES)
    yield d
    shutil.rmtree(d, ignore_errors=True)


ON_DEVICE = [c for c in CASES["cases"] if c["device"]]


@pytest.mark.parametrize("case", ON_DEVICE, ids=lambda c: c["id"])
def test_every_golden_replays_on_the_gpu(case, workdir):
    assert len(ON_DEVICE) >= 40 and sum(c["trained"] for c in ON_DEVICE) >= 12
    p = subprocess.run([U.BINARY] + case["argv"], cwd=workdir, capture_output=True, timeout=300)
    err = p.stderr.decode("latin-1")
    assert p.returncode == case["exit"], err[-500:]
    its = U.iterations(p.stderr)
    differ = [(i + 1, a, b) for i, (a, b) in enumerate(zip(its, case["iterations"])) if abs(float(a) - float(b)) > 2e-6]
    worst = max([abs(float(a) - float(b)) for a, b in zip(its, case["iterations"])], default=0.0)
    print("%s: %d iterations, largest difference %.3g" % (case["id"], len(its), worst))
    assert not differ, "iteration %d: %s here, %s in the reference (%d more differ)" % (differ[0] + (len(differ) - 1,))
    assert len(its) == len(case["iterations"]) and (len(its) > 7) == case["trained"]
    assert U.stdout_matches(case, p.stdout), (case["id"], p.stdout[:400])
    assert [l for l in err.split("\n") if l.startswith("Y inconsistency") or l.startswith("No calls")] == case["stderr_lines"]


def test_pipeline_counter_into_caller(tmp_path):
    pipe = CASES["pipeline"]
    (tmp_path / "db.txt").write_bytes(U.pipeline_db())
    (tmp_path / "reads.fq").write_bytes(GU.big_reads())
    c = subprocess.run([U.COUNTER, "-db", "db.txt", "reads.fq"], cwd=tmp_path, capture_output=True, timeout=300)
    assert c.returncode == 0 and (U.sha(c.stdout), len(c.stdout)) == (pipe["counts_sha256"], pipe["counts_bytes"]), c.stderr
    (tmp_path / "counts.txt").write_bytes(c.stdout)
    p = subprocess.run([U.BINARY] + pipe["argv"], cwd=tmp_path, capture_output=True, timeout=300)
    assert p.returncode == pipe["exit"] and p.stderr == b""
    assert U.stdout_matches(pipe, p.stdout) and p.stdout.count(b"\n") > 1000
