"""The device reader (gt4hip_maker.hip, gt4hip_maker_tile.h, and k_mk_text_counts of gt4hip_gmer.hip on the same tile_head)
with the structural bytes of FastA / FastQ on the edges of its geometry: the texts of tests/reader_texts.py (held to what they
promise by tests/test_reader_texts_model.py) through the C ABI's four text entry points, against the byte-serial models --
exactly, this is integer work.  A thread takes P = 16 bytes, a wavefront W = 1024, a tile T = 4096; k_mk_state_scan gives each of
its 1024 threads a stretch of tiles, of more than one tile only for a text of more than 1024 tiles (the `units` tests).

Every sweep test takes one edge and one kind of pad, about 150 to 250 texts; the largest (the edge at 2 T, with a tile of
ordinary records behind it) are texts of 3 T + 250 bytes."""
import numpy as np
import pytest

import gmer_model as GM
import index_model as IM
import maker_model as M
import query_model as QM
import reader_texts as R
import seqprofile_model as SP
from genometester4_amd.listio import make_records

pytestmark = pytest.mark.gpu

from genometester4_amd import capi  # noqa: E402

U64 = np.uint64
STAT_FIELDS = ("n_n", "n_nucl", "n_gc", "n_words", "n_hits", "n_kmer_gc")


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    # no counter reports a thread's bytes: a change of geometry fails here instead of moving the edges away from the probes
    assert c.get_counter("maker_text_tile") == 256 * 16 == R.T and (R.P, R.W, R.SCAN) == (16, 64 * 16, 1024)
    yield c
    c.close()


def same(got, want, *where):
    """two uint64 arrays are equal; the message names the first place where they are not"""
    want, got = np.asarray(want, dtype=U64), np.asarray(got)
    if got.size == 0 and want.size == 0:
        return
    if got.shape != want.shape or not np.array_equal(got, want):
        n = min(len(got), len(want))
        diff = np.flatnonzero(got[:n] != want[:n]) if got.ndim == 1 else np.flatnonzero((got[:n] != want[:n]).any(axis=1))
        at = int(diff[0]) if len(diff) else n
        pytest.fail("%r: %d entries for %d, the first difference at %d: %s for %s" % (where, len(got), len(want), at, got[at:at + 2].tolist(), want[at:at + 2].tolist()))


def check_words(ctx, text, k, flags, *where):
    want, err = M.read_words(text, k, canonize=not (flags & capi.MAKER_FORWARD_ONLY))
    assert err is None
    got, carry = ctx.text_to_words(text, k, flags)
    same(got, want, "words", k, *where)
    return carry


def model_locations(text, k):
    words, ords, poss, dirs, subs = IM.read_locations(text, k)
    return words, [(o << 33) | (p << 1) | d for o, p, d in zip(ords, poss, dirs)], subs, max(poss) if poss else 0


def check_locations(ctx, text, k, *where, model_text=None):
    words, raw, subs, max_pos = model_locations(text if model_text is None else model_text, k)
    got = ctx.text_to_locations([text], k)
    same(got[0], words, "words beside locations", k, *where)
    same(got[1], raw, "raw locations", k, *where)
    assert got[2] == subs, ("subsequences", k) + where
    assert got[3] == max_pos, ("largest position", k) + where


class Db:
    """a gmer_model.Database and the same k-mers on the device"""

    def __init__(self, ctx, dbm):
        self.model, self.dev = dbm, ctx.gmer_db(np.array([w for ws in dbm.words for w in ws], dtype=U64), dbm.wordsize)

    def count(self, pieces):
        """(statistics summed over the pieces of one text, the counters)"""
        self.dev.reset()
        total, carry = dict.fromkeys(STAT_FIELDS, 0), None
        for p in pieces:
            st, carry = self.dev.count_text(p, carry)
            for f in STAT_FIELDS:
                total[f] += getattr(st, f)
        return total, self.dev.counts(), carry

    def check(self, text, *where, model_text=None):
        counts, st, err = GM.count(self.model, [text if model_text is None else model_text])
        assert err is None
        got, got_counts, carry = self.count([text])
        assert got == st, where
        same(got_counts, counts, "k-mer counts", *where)
        return st, carry


@pytest.fixture(scope="module")
def dbs(ctx):
    """per kind, every other 5-mer of the sweeps' tail"""
    d = {kind: Db(ctx, R.database(R.tail(kind))) for kind in R.KINDS}
    assert all(db.model.n_kmers > 100 for db in d.values())
    yield d
    for db in d.values():
        db.dev.free()


@pytest.fixture(scope="module")
def five_mers(ctx):
    """every other canonical 5-mer with a count, as a list on the device with its query index"""
    keys = np.unique(QM.canonical_np(np.arange(1 << 10, dtype=U64), 5))[::2]
    counts = (np.arange(len(keys)) % 50 + 1).astype(np.uint32)
    ix = ctx.upload(make_records(keys, counts), 5).query_index()
    yield keys, counts, ix
    ix.free()


def check_profile(ctx, listed, text, k, *where):
    keys, counts, ix = listed
    _, want = SP.profile_text(keys, counts, text, k)
    got, subs = ctx.query_profile_text(ix, [text])
    same(np.stack([got["n_words"], got["n_hits"], got["sum"]], axis=1) if len(got) else np.zeros((0, 3), dtype=U64), want, "words, hits and sum per sequence", *where)
    assert subs == IM.read_locations(text, k)[4], where


# ------------------------------------------------------------------ sweeps

SWEEPS = [(kind, edge, pad) for kind in R.KINDS for edge in R.EDGES for pad in R.PAD_KINDS[kind]]
WHATS = ("words-k32", "words-k1-forward", "locations-k32", "locations-k5", "counts")


@pytest.mark.parametrize("what", WHATS)
@pytest.mark.parametrize("kind,edge,pad", SWEEPS, ids=["%s-%s-%s" % s for s in SWEEPS])
def test_probe_swept_over_an_edge(ctx, dbs, kind, edge, pad, what):
    """each byte of the probe (and of what closes the pad's record) once the last byte before the edge and once the first behind it"""
    n = hits = 0
    for at, text in R.sweep(kind, R.EDGES[edge], pad):
        if what == "words-k32":
            check_words(ctx, text, 32, 0, at)
        elif what == "words-k1-forward":
            check_words(ctx, text, 1, capi.MAKER_FORWARD_ONLY, at)
        elif what == "counts":
            hits += dbs[kind].check(text, at)[0]["n_hits"]
        else:
            check_locations(ctx, text, int(what[11:]), at)
        n += 1
    assert n > 16 and (what != "counts" or hits > n * 100)


# ------------------------------------------------------------------ hostile variants

@pytest.mark.parametrize("edge", R.HOSTILE_EDGES)
@pytest.mark.parametrize("variant", R.HOSTILE)
def test_changed_byte_swept_over_an_edge(ctx, dbs, variant, edge):
    """a missing tag is the model's error at the model's offset from every entry point; a NUL ends the text, and what lies
    behind it (a record without its '+' line among it) is not read"""
    kind, _, _, _, want = R.HOSTILE[variant]
    k, n = 8, 0
    for at, text in R.hostile(variant, R.EDGES[edge]):
        assert M.read_words(text, k)[1] == (None if want is None else (want, at))
        if want is None:
            cut = text[:at]
            same(ctx.text_to_words(text, k)[0], M.read_words(cut, k)[0], "words in front of the NUL", at)
            assert check_words(ctx, text, 3, capi.MAKER_FORWARD_ONLY, at).ended == 1
            check_locations(ctx, text, k, at, model_text=cut)
            _, carry = dbs[kind].check(text, at, model_text=cut)
            assert carry.ended == 1
            ctx.text_to_list(text, k).free()  # (the whole-text entry point finds no error either)
        else:
            for call in (lambda: ctx.text_to_words(text, k), lambda: ctx.text_to_locations([text], k), lambda: dbs[kind].dev.count_text(text)):
                with pytest.raises(capi.Gt4HipError) as e:
                    call()
                assert (e.value.code, e.value.kind, e.value.error_offset) == (capi.EFORMAT, want, at), at
            with pytest.raises(capi.Gt4HipError) as e:
                ctx.text_to_list(text, k)
            assert e.value.code == capi.EFORMAT, at
            if want == M.ERR_PLUS_EOF:
                # the same without the NUL: a piece that ends inside a '+' line may go on, a whole text may not
                assert M.read_words(text[:at], k)[1] == (want, at)
                assert ctx.text_to_words(text[:at], k)[1].ended == 0
                with pytest.raises(capi.Gt4HipError) as e:
                    ctx.text_to_list(text[:at], k)
                assert e.value.code == capi.EFORMAT and "'+' line" in str(e.value), at
        n += 1
    assert n > 60


# ------------------------------------------------------------------ grammar

@pytest.mark.parametrize("what", ("words", "locations", "counts", "profile"))
@pytest.mark.parametrize("kind", R.KINDS)
def test_texts_drawn_from_a_grammar(ctx, dbs, five_mers, kind, what):
    for seed in R.SEEDS:
        text = R.grammar(seed, kind)
        if what == "words":
            check_words(ctx, text, 32, 0, seed)
            check_words(ctx, text, 1, capi.MAKER_FORWARD_ONLY, seed)
        elif what == "locations":
            check_locations(ctx, text, 32, seed)
            check_locations(ctx, text, 5, seed)
        elif what == "counts":
            dbs[kind].check(text, seed)
        elif seed % 10 == 0:
            check_profile(ctx, five_mers, text, 5, seed)


# ------------------------------------------------------------------ units: more tiles than k_mk_state_scan has threads

UNITS_K = 25
_units = {}


def the_units(kind):
    """(text of N_UNITS units and the long-named record, what the models give for it, its parts)"""
    if kind not in _units:
        parts = R.units(kind)
        text = R.units_text(parts)
        assert -(-len(text) // R.T) > R.SCAN
        _units[kind] = (text, R.units_expected(parts, UNITS_K), parts)
    return _units[kind]


def pieces_of(text):
    cuts = R.units_cuts()
    return [text[a:b] for a, b in zip([0] + cuts, cuts + [len(text)])]


@pytest.mark.parametrize("pieces", ["whole", "three-pieces"])
@pytest.mark.parametrize("kind", R.KINDS)
def test_units_words(ctx, kind, pieces):
    text, e, _ = the_units(kind)
    got, carry = [], None
    for p in [text] if pieces == "whole" else pieces_of(text):
        w, carry = ctx.text_to_words(p, UNITS_K, carry=carry)
        got.append(w)
    same(np.concatenate(got), e["words"], "words", kind, pieces)


@pytest.mark.parametrize("pieces", ["whole", "three-pieces"])
@pytest.mark.parametrize("kind", R.KINDS)
def test_units_locations(ctx, kind, pieces):
    text, e, _ = the_units(kind)
    words, raw, subs, max_pos = ctx.text_to_locations([text] if pieces == "whole" else pieces_of(text), UNITS_K)
    same(words, e["words"], "words beside locations", kind, pieces)
    same(raw, R.raw_locations(e), "raw locations", kind, pieces)
    same(np.array(subs, dtype=U64), e["subseqs"], "subsequences", kind, pieces)
    assert max_pos == int(e["positions"].max())


@pytest.mark.parametrize("pieces", ["whole", "three-pieces"])
@pytest.mark.parametrize("kind", R.KINDS)
def test_units_counts(ctx, kind, pieces):
    """the sums and the counters are the parts' own, added up"""
    text, _, parts = the_units(kind)
    db = Db(ctx, R.database(parts[0][0], UNITS_K))
    try:
        want, want_counts = dict.fromkeys(STAT_FIELDS, 0), np.zeros(db.model.n_kmers, dtype=U64)
        for part, n in ((parts[0][0], parts[0][1] + parts[2][1]), (parts[1][0], 1)):
            counts, st, err = GM.count(db.model, [part])
            assert err is None
            for f in STAT_FIELDS:
                want[f] += n * st[f]
            want_counts += U64(n) * np.array(counts, dtype=U64)
        assert want["n_hits"] > R.N_UNITS * 500 and want["n_n"] > R.N_UNITS
        got, got_counts, _ = db.count([text] if pieces == "whole" else pieces_of(text))
        assert got == want
        same(got_counts, want_counts, "k-mer counts", kind, pieces)
    finally:
        db.dev.free()


@pytest.mark.parametrize("pieces", ["whole", "three-pieces"])
@pytest.mark.parametrize("kind", R.KINDS)
def test_units_profile(ctx, kind, pieces):
    """words, hits and sum per sequence: the parts' own rows, repeated"""
    text, e, parts = the_units(kind)
    words = np.unique(np.array(IM.read_locations(parts[0][0], UNITS_K)[0], dtype=U64))
    keys = np.unique(np.concatenate([words[::2], QM.canonical_np(np.arange(1000, 1100, dtype=U64), UNITS_K)]))
    counts = (np.arange(len(keys)) % 50 + 1).astype(np.uint32)
    ix = ctx.upload(make_records(keys, counts), UNITS_K).query_index()
    try:
        want = np.concatenate([np.tile(SP.profile_text(keys, counts, part, UNITS_K)[1], (rep, 1)) for part, rep in parts])
        assert np.array_equal(want[:, 0], np.bincount(e["ordinals"].astype(np.int64), minlength=len(e["subseqs"])).astype(U64)) and want[:, 1].sum() > R.N_UNITS * 500
        got, subs = ctx.query_profile_text(ix, [text] if pieces == "whole" else pieces_of(text))
        same(np.stack([got["n_words"], got["n_hits"], got["sum"]], axis=1), want, "words, hits and sum per sequence", kind, pieces)
        same(np.array(subs, dtype=U64), e["subseqs"], "subsequences", kind, pieces)
    finally:
        ix.free()
