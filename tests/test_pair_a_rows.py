"""The A-rows body of the A-only pair kernels (intersection, first complement: gt4hip_kernels.hip, A_ROWS) at the edges of its
per-tile test `na <= NT * (IPT / 2)`.

The two lists are built block by block, one block per merge tile: tile boundaries are the diagonals at multiples of
T = NT * IPT - 64 of the merged order (A first on ties), so a block of s shared, ao A-only and bo B-only keys with
2 s + ao + bo = T that ends on an unshared key IS a tile, with exactly na = s + ao A records.  One launch holds tiles with
na = H - 1, H, H + 1 (H = NT * IPT / 2: the cutoff of the branch), H - 64, H - 63 (the last chunk of the last A row empty /
one record), 0, 1, 64, T / 2, T and a short last tile.  The CPU part recomputes every tile's na from the key arrays alone and
asserts that these values occur; the GPU part runs -i, -i -c 2, -d, -d -c 2 and three-list intersect_multi chains on them, on
the single-pass and the two-pass path and count-only, with option "a_rows" 0 (the body chosen per tile) and -1 (always the
general body), against the CPU oracle: records, n_words, total_count.  A second set of lists has key gaps that make a tile
span more than 2^32 (the full-width match test), with k = 32 keys over the whole 64-bit range."""
import functools

import numpy as np
import pytest

import oracle_lib as O
from genometester4_amd.listio import make_records

U32 = 0xFFFFFFFF
C_EDGE = 2  # the cutoff of the -c 2 calls: the drawn counts sit around it

# (name, NT, IPT, options that select the geometry): 1024 x 6 the intersection, 1024 x 4 the first complement, 512 x 4 the
# intersection and the complement under "geom0" and every count-only call
GEOMS = {"1024x6": (1024, 6), "1024x4": (1024, 4), "512x4": (512, 4)}


def tile_T(nt, ipt):
    return nt * ipt - 64


def na_targets(nt, ipt):
    T, H = tile_T(nt, ipt), nt * ipt // 2
    return [H - 1, T // 2, H, 0, H + 1, 1, H - 64, T, H - 63, 64]


def edge_counts(rng, n, c=C_EDGE):
    """zeros and values around the cutoff and the ends of u32, half of them small (as tests/test_count_edges.py's inputs)"""
    edges = np.array([0, 1, c - 1, c, c + 1, (1 << 31) - 1, 1 << 31, U32 - 1, U32], dtype=np.uint64).astype(np.uint32)
    out = edges[rng.integers(0, len(edges), n)]
    small = rng.random(n) < 0.5
    out[small] = rng.integers(0, 6, int(small.sum()), dtype=np.uint32)
    return out


def block_keys(rng, nas, T, last, first_key, step, wide):
    """Keys of two lists, one block per entry of nas (+ a short last block of `last` = (na, nb) records): returns (ka, kb).
    step: spacing of the universe keys (room for neighbours, see chain lists); wide: a gap of 2^33 in the middle of every block"""
    ka, kb = [], []
    key = first_key
    for j, v in enumerate(list(nas) + [None]):
        if v is None:
            na, nb = last
            s = min(na, nb) // 2
        else:
            na, nb = v, T - v
            s = (min(na, nb) + 1) // 2
        ao, bo = na - s, nb - s
        n = s + ao + bo
        assert ao + bo >= 1
        kind = np.concatenate([np.zeros(s, np.int8), np.ones(ao, np.int8), np.full(bo, 2, np.int8)])
        rng.shuffle(kind)
        if kind[-1] == 0:  # a block ends on an unshared key: no pair straddles a tile boundary
            i = int(np.flatnonzero(kind != 0)[-1])
            kind[i], kind[-1] = kind[-1], kind[i]
        gaps = rng.integers(1, 4, n, dtype=np.uint64) * np.uint64(step)
        if wide:
            gaps[n // 2] += np.uint64(1) << np.uint64(33)
        keys = np.uint64(key) + np.cumsum(gaps, dtype=np.uint64)
        key = int(keys[-1])
        ka.append(keys[kind != 2])
        kb.append(keys[kind != 1])
    return np.concatenate(ka), np.concatenate(kb)


def tile_nas(ka, kb, T):
    """A records of every merge tile, from the keys alone: co-ranks along the diagonals j * T of the merged order, A first on
    ties (the B record of a pair cut off by a diagonal moves to the earlier tile: that changes nb, not na)"""
    rank_a = np.arange(len(ka)) + np.searchsorted(kb, ka, side="left")
    total = len(ka) + len(kb)
    diag = np.minimum(np.arange((total + T - 1) // T + 1) * T, total)
    a = np.searchsorted(rank_a, diag, side="left")
    return np.diff(a)


@functools.lru_cache(maxsize=None)
def lists(geom, wide):
    """(k, A, B, C, L0, L1): A, B the block pair of the geometry; the chain lists: intersect_multi (A, B, C) meets the blocks at
    its first step (FAST 2); intersect_multi (L0, L1, B) with L0 n L1 = A's keys meets them at its last (FAST 3)"""
    nt, ipt = GEOMS[geom]
    T = tile_T(nt, ipt)
    rng = np.random.default_rng(1000 * nt + 10 * ipt + (1 if wide else 0))
    k = 32 if wide else 25
    first = 0 if wide else 12345
    ka, kb = block_keys(rng, na_targets(nt, ipt), T, (100, 217), first, 4, wide)
    if wide:
        # k = 32: the whole 64-bit range -- the upper half of the keys moved up against 2^64
        shift = np.uint64((1 << 64) - 4 - int(max(ka[-1], kb[-1])))
        thr = ka[len(ka) // 2]
        ka = np.where(ka >= thr, ka + shift, ka)
        kb = np.where(kb >= thr, kb + shift, kb)
    assert len(ka) <= len(kb)  # (an intersection searches with its shorter list: A stays A)
    A = make_records(ka, edge_counts(rng, len(ka)))
    B = make_records(kb, edge_counts(rng, len(kb)))
    both = np.union1d(ka, kb)
    kc = both[rng.random(len(both)) < 0.7]
    C = make_records(kc, edge_counts(rng, len(kc)))
    # L0, L1: A's keys plus neighbours of their own (universe keys are 4 apart: + 1 and + 2 are free, in B too)
    e0 = ka[rng.random(len(ka)) < 0.3] + np.uint64(1)
    e1 = ka[rng.random(len(ka)) < 0.3] + np.uint64(2)
    k0, k1 = np.union1d(ka, e0), np.union1d(ka, e1)
    # counts >= 1 on A's keys: the running minimum of the chain then is the plain minimum, never 0 (a 0 restarts it)
    L0 = make_records(k0, edge_counts(rng, len(k0)) | np.uint32(1))
    L1 = make_records(k1, edge_counts(rng, len(k1)) | np.uint32(1))
    return k, A, B, C, L0, L1


WIDE = (False, True)


@pytest.mark.parametrize("wide", WIDE, ids=["narrow", "wide"])
@pytest.mark.parametrize("geom", list(GEOMS))
def test_tiles_hit_the_edges_of_the_branch(geom, wide):
    nt, ipt = GEOMS[geom]
    T, H = tile_T(nt, ipt), nt * ipt // 2
    k, A, B, C, L0, L1 = lists(geom, wide)
    for rec in (A, B, C, L0, L1):
        assert rec["key"].dtype == np.uint64 and (rec["key"][1:] > rec["key"][:-1]).all()
    nas = tile_nas(A["key"], B["key"], T)
    assert list(nas[:-1]) == na_targets(nt, ipt) and nas[-1] == 100, nas
    assert {H - 1, H, H + 1, H - 64, H - 63, 0, 1, 64, T // 2, T} <= set(int(x) for x in nas)
    assert len(A) + len(B) < 100_000
    # the last step of the (L0, L1, B) chain runs on A's keys again
    assert np.array_equal(np.intersect1d(L0["key"], L1["key"]), A["key"])
    # span of the keys of every tile: below 2^32 in the narrow lists, above in every tile of the wide ones
    bounds = np.concatenate([[0], np.cumsum(nas)])
    rank_b = np.concatenate([[0], np.cumsum(np.append(T - nas[:-1], 317 - nas[-1]))])
    for j in range(len(nas)):
        ks = np.concatenate([A["key"][bounds[j]:bounds[j + 1]], B["key"][rank_b[j]:rank_b[j + 1]]])
        span = int(ks.max()) - int(ks.min())
        assert (span >> 32 != 0) == wide, (j, span)
    if wide:
        assert int(B["key"][-1]) >> 63 == 1 or int(A["key"][-1]) >> 63 == 1


@pytest.fixture(scope="module")
def ctx():
    from genometester4_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def dev(ctx):
    made = {}

    def get(geom, wide):
        if (geom, wide) not in made:
            k, *recs = lists(geom, wide)
            made[(geom, wide)] = [ctx.upload(r, k) for r in recs]
        return made[(geom, wide)]
    return get


@functools.lru_cache(maxsize=None)
def oracle_pair(geom, wide, ops, cutoff):
    k, A, B, *_ = lists(geom, wide)
    return O.compare(A, B, ops, 0, cutoff)[ops]


@functools.lru_cache(maxsize=None)
def oracle_chain(geom, wide, which, cutoff):
    k, A, B, C, L0, L1 = lists(geom, wide)
    return O.intersect_multi([A, B, C] if which == 0 else [L0, L1, B], cutoff)


# (id, options, count_only); the geometry's own options are added
PATHS = (("single_pass", {}, False), ("two_pass", {"two_pass": 1}, False), ("count_only", {}, True))
RESET = {"two_pass": 0, "geom0": 0, "geom1": 0, "a_rows": 0}


def geom_options(geom, ops, count_only):
    """the options under which a call of `ops` runs in the geometry: 1024 x 6 is the intersection's own, 1024 x 4 the
    complement's; 512 x 4 is "geom0" (count-only calls take it by themselves)"""
    nt, ipt = GEOMS[geom]
    if nt == 512:
        return {} if count_only else {"geom0": 1}
    if (ipt == 6) != (ops == 2):
        return None  # not a geometry of this class
    return {"geom1": 1} if count_only else {}


def _set(ctx, opts):
    for name, value in opts.items():
        ctx.set_option(name, value)


CALLS = [(ops, cutoff) for ops in (2, 4) for cutoff in (1, C_EDGE)]  # -i, -i -c 2, -d, -d -c 2


@pytest.mark.gpu
@pytest.mark.parametrize("a_rows", (0, -1))
@pytest.mark.parametrize("path", PATHS, ids=[p[0] for p in PATHS])
@pytest.mark.parametrize("wide", WIDE, ids=["narrow", "wide"])
@pytest.mark.parametrize("geom", list(GEOMS))
def test_pair_calls(ctx, dev, geom, wide, path, a_rows):
    _, opts, count_only = path
    ran = 0
    for ops, cutoff in CALLS:
        g = geom_options(geom, ops, count_only)
        if g is None:
            continue
        ran += 1
        n_o, t_o, r_o = oracle_pair(geom, wide, ops, cutoff)
        d = dev(geom, wide)
        try:
            _set(ctx, dict(opts, a_rows=a_rows, **g))
            st, out, timing = ctx.compare(d[0], d[1], ops, 0, cutoff, 0, 1, count_only)
        finally:
            _set(ctx, RESET)
        nt, ipt = GEOMS[geom]
        assert timing["merge_tiles"] == len(na_targets(nt, ipt)) + 1, (timing, geom, ops)  # the geometry the blocks were cut for
        assert st[ops] == (n_o, t_o), (geom, wide, path[0], a_rows, ops, cutoff, st[ops], (n_o, t_o))
        if not count_only:
            got = out[ops].download()
            out[ops].free()
            assert got.tobytes() == r_o.tobytes(), (geom, wide, path[0], a_rows, ops, cutoff)
    assert ran >= 2


@pytest.mark.gpu
@pytest.mark.parametrize("a_rows", (0, -1))
@pytest.mark.parametrize("path", PATHS, ids=[p[0] for p in PATHS])
@pytest.mark.parametrize("wide", WIDE, ids=["narrow", "wide"])
@pytest.mark.parametrize("geom", ("1024x6", "512x4"))
def test_intersect_multi_chains(ctx, dev, geom, wide, path, a_rows):
    _, opts, count_only = path
    g = geom_options(geom, 2, count_only)
    d = dev(geom, wide)
    for which, cutoff in ((0, 1), (1, C_EDGE), (1, 1)):
        rc_o, n_o, t_o, r_o = oracle_chain(geom, wide, which, cutoff)
        assert rc_o == 0
        three = [d[0], d[1], d[2]] if which == 0 else [d[3], d[4], d[1]]
        try:
            _set(ctx, dict(opts, a_rows=a_rows, **g))
            rc, n_g, t_g, out = ctx.intersect_multi(three, cutoff, 0, 1, count_only)
        finally:
            _set(ctx, RESET)
        assert rc == 0
        assert (n_g, t_g) == (n_o, t_o), (geom, wide, path[0], a_rows, which, cutoff, (n_g, t_g), (n_o, t_o))
        if not count_only:
            got = out.download()
            out.free()
            assert got.tobytes() == r_o.tobytes(), (geom, wide, path[0], a_rows, which, cutoff)
