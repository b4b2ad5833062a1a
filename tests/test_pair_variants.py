"""Every launchable k_pair_merge<...> instantiation, reached by construction (tests/pair_variants.py says which call and
path takes which; tests/test_pair_variant_map.py ties that map to the compiled set), checked byte for byte against the
CPU oracle: n_words, total_count and the records of every stream, on inputs long enough that every geometry runs more
tiles than the resident grid holds, with counts at the edges of u32 arithmetic (ADD wrapping to exactly 0 and 1,
cutoffs 0, 1, 3 and 2^32 - 1)."""
import numpy as np
import pytest

import oracle_lib as O
import pair_variants as V
from genometester4_amd.listio import make_records

pytestmark = pytest.mark.gpu

BIG = 3_400_000        # records per list of the large pairs
MIN_TOTAL = 6_500_000  # per pair: more than 1,000 tiles of the longest tile (6,080 records)
U32 = 0xFFFFFFFF
C_EDGE = 3             # the cutoff the drawn count extremes sit around


@pytest.fixture(scope="module")
def ctx():
    from genometester4_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def edge_counts(rng, n, c=C_EDGE):
    """half from {0, 1, 2, c-1, c, c+1, 2^31-1, 2^31, 2^32-2, 2^32-1}, half small (0..8)"""
    edges = np.array([0, 1, 2, c - 1, c, c + 1, (1 << 31) - 1, 1 << 31, U32 - 1, U32], dtype=np.uint64).astype(np.uint32)
    out = edges[rng.integers(0, len(edges), n)]
    small = rng.random(n) < 0.5
    out[small] = rng.integers(0, 9, int(small.sum()), dtype=np.uint32)
    return out


def _pick(rng, keys, p):
    return keys[rng.random(len(keys)) < p]


def _shared_sums(a, b):
    _, ia, ib = np.intersect1d(a["key"], b["key"], assume_unique=True, return_indices=True)
    return a["count"][ia].astype(np.uint64) + b["count"][ib].astype(np.uint64)


def _main_lists(ctx):
    """synth.make_pair(dist="iid") keys with the edge counts, and three more lists over the same keys for the N-way calls"""
    from genometester4_amd import synth
    a, b = synth.make_pair(ctx, BIG, 25, dist="iid", seed=5)
    ha, hb = a.download(), b.download()
    a.free()
    b.free()
    rng = np.random.default_rng(11)
    ha["count"] = edge_counts(rng, len(ha))
    hb["count"] = edge_counts(rng, len(hb))
    # shared keys that meet the wrap exactly: 2^32 (ADD is 0: dropped), 2^32 + 1, 2^31 + 2^31
    sums = _shared_sums(ha, hb)
    assert (sums == 1 << 32).sum() > 1000 and (sums == (1 << 32) + 1).sum() > 1000
    universe = np.union1d(ha["key"], hb["key"])
    lists = [ha, hb]
    for j in range(3):
        keys = _pick(rng, universe, 0.7)
        lists.append(make_records(keys, edge_counts(rng, len(keys))))
    return 25, lists


def _universe_pair(seed, k, n_universe, lo=0, hi=None, p=(0.67, 0.67), ends=False):
    """host-made pair out of one universe; classes as synth's: A, B each about p of it"""
    rng = np.random.default_rng(seed)
    hi = hi if hi is not None else (1 << (2 * k))
    if hi > 1 << 63:
        keys = rng.integers(0, 1 << 63, n_universe, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n_universe, dtype=np.uint64)
    else:
        keys = rng.integers(lo, hi, n_universe, dtype=np.uint64)
    if ends:
        keys = np.concatenate([keys, np.array([0, (1 << 64) - 1], dtype=np.uint64)])
    keys = np.unique(keys)
    cls = rng.integers(0, 3, len(keys))
    if ends:
        cls[0] = cls[-1] = 1  # 0 and 2^64 - 1 in both lists
    ka, kb = keys[cls <= 1], keys[cls >= 1]
    return make_records(ka, edge_counts(rng, len(ka))), make_records(kb, edge_counts(rng, len(kb)))


def _ragged(seed):
    """10 : 1 -- most tiles are all A, some all B; most of B's keys lie in A"""
    rng = np.random.default_rng(seed)
    keys = np.unique(rng.integers(0, 1 << 40, 6_700_000, dtype=np.uint64))
    in_a = rng.random(len(keys)) < 0.9
    ka = keys[in_a]
    kb = np.union1d(_pick(rng, ka, 0.07), _pick(rng, keys[~in_a], 0.3))
    return make_records(ka, edge_counts(rng, len(ka))), make_records(kb, edge_counts(rng, len(kb)))


@pytest.fixture(scope="module")
def inputs(ctx):
    """{name: (k, host lists, device lists)}, built once"""
    from genometester4_amd import synth
    made = {"main": _main_lists(ctx)}
    for dist in ("genomic", "clustered"):
        a, b = synth.make_pair(ctx, BIG, 25, dist=dist, seed=7)
        made[dist] = (25, [a.download(), b.download()])
        a.free()
        b.free()
    made["dense16"] = (16, list(_universe_pair(13, 16, 5_100_000, hi=1 << 28)))
    made["k32"] = (32, list(_universe_pair(17, 32, 5_000_000, hi=1 << 64, ends=True)))
    ra, rb = _ragged(19)
    made["ragged_ab"] = (20, [ra, rb])
    made["ragged_ba"] = (20, [rb, ra])
    out = {}
    for name, (k, lists) in made.items():
        assert len(lists[0]) + len(lists[1]) >= MIN_TOTAL, (name, len(lists[0]), len(lists[1]))
        for h in lists:
            assert np.all(h["key"][1:] > h["key"][:-1]), name
        out[name] = (k, lists, [ctx.upload(h, k) for h in lists])
    assert out["k32"][1][0]["key"][0] == 0 and out["k32"][1][1]["key"][-1] == (1 << 64) - 1
    assert np.all(out["dense16"][1][1]["key"] < 1 << 32)
    return out


_last = {}


def _oracle(key, fn):
    """the oracle's result of one (input, call), computed once for all paths of it (the cases run call by call)"""
    if key not in _last:
        _last.clear()
        _last[key] = fn()
    return _last[key]


def _set(ctx, opts):
    for name, value in opts.items():
        ctx.set_option(name, value)


def _reset(ctx):
    _set(ctx, V.RESET)


def _run_pair(ctx, inputs, name, call, path):
    ops, rule, cutoff, sub = call
    _, host, dev = inputs[name]
    exp = _oracle((name,) + call, lambda: O.compare(host[0], host[1], ops, rule, cutoff, sub))
    opts, _ = V.path_options(path, ops)
    count_only, two_pass, geom = V.path_geometry(path)
    try:
        _set(ctx, opts)
        st, out, timing = ctx.compare(dev[0], dev[1], ops, rule, cutoff, sub, 1, count_only)
    finally:
        _reset(ctx)
    launch = V.compare_launches(ops, rule, cutoff, sub, len(host[0]), len(host[1]), count_only=count_only, two_pass=two_pass, geom=geom)
    # the geometry and tile length the map predicts are the ones the host took
    assert timing["merge_tiles"] == launch.tiles and launch.tiles >= 1000, (timing["merge_tiles"], launch)
    for bit in (1, 2, 4, 8):
        if not ops & bit:
            continue
        assert st[bit] == exp[bit][:2], (name, call, path, bit, st[bit], exp[bit][:2])
        if not count_only:
            got = out[bit].download()
            assert got.tobytes() == exp[bit][2].tobytes(), "stream %d differs from the oracle (%s, %s, %s)" % (bit, name, call, path)
            out[bit].free()


PAIR_CASES = [(c[1:], path) for c, path in V.matrix() if c[0] == "pair"]
MULTI_CASES = [(c, path) for c, path in V.matrix() if c[0] != "pair"]


def _id(call, path):
    return "%s-%s" % ("_".join(str(x) for x in call), path)


@pytest.mark.parametrize("call,path", PAIR_CASES, ids=[_id(c, p) for c, p in PAIR_CASES])
def test_pair_variant(ctx, inputs, call, path):
    _run_pair(ctx, inputs, "main", call, path)


@pytest.mark.parametrize("call,path", MULTI_CASES, ids=[_id(c, p) for c, p in MULTI_CASES])
def test_nway_variant(ctx, inputs, call, path):
    entry, n, rule, cutoff = call
    host = inputs["main"][1][:n]
    rc, n_o, t_o, r_o = _oracle(call, lambda: (O.union_multi if entry == "union_multi" else O.intersect_multi)(host, cutoff, rule))
    assert rc == 0
    dev = inputs["main"][2][:n]
    opts, count_only = V.path_options(path, 0)
    opts["kway"] = 0  # union_multi by the pairwise tree of the pair kernel (FILTER_RAW / FILTER_RESULT levels)
    fn = ctx.union_multi if entry == "union_multi" else ctx.intersect_multi
    try:
        _set(ctx, opts)
        rc, n_g, t_g, out = fn(dev, cutoff, rule, 1, count_only)
    finally:
        _reset(ctx)
    assert rc == 0
    assert (n_g, t_g) == (n_o, t_o), (call, path, (n_g, t_g), (n_o, t_o))
    if not count_only:
        assert out.download().tobytes() == r_o.tobytes(), (call, path)
        out.free()


SIDE_INPUTS = ("genomic", "clustered", "dense16", "k32", "ragged_ab", "ragged_ba")
SIDE_CASES = [(name, c, path) for name in SIDE_INPUTS for c in V.SIDE_CALLS for path in V.SIDE_PATHS]


@pytest.mark.parametrize("name,call,path", SIDE_CASES, ids=["%s-%s" % (n, _id(c, p)) for n, c, p in SIDE_CASES])
def test_pair_variant_other_inputs(ctx, inputs, name, call, path):
    _run_pair(ctx, inputs, name, call, path)
