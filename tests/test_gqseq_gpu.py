"""gt4hip_seqprofile.hip at the library level through capi, against tests/seqprofile_model.py (held to the reference in
tests/test_gqseq_model.py), at the smallest shapes where the kernel can go wrong: runs of equal ordinal that end at the edges
of a tile, of a round, of a wavefront and at lanes 0 / 63, sequences without words, both templates.  The module's context
runs with option "poison": the sums are zeroed by the call, never by what a pooled block held."""
import numpy as np
import pytest

import index_model
import query_model as QM
import seqprofile_model as SP
from genometester4_amd.listio import make_records

pytestmark = pytest.mark.gpu

WAVE = 64
EINVAL, EFORMAT = 1, 11


@pytest.fixture(scope="module")
def ctx():
    from genometester4_amd import capi
    c = capi.Context(0)
    c.set_option("poison", 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def T(ctx):
    t = ctx.get_counter("profile_tile")
    assert t % ctx.get_counter("mm_threads") == 0 and t > WAVE
    return t


@pytest.fixture(scope="module")
def W(ctx):
    return ctx.get_counter("mm_threads")


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()


_lists = {}


def the_list(k, n_keys, seed):
    """canonical words ascending, a count each: zeros and all-ones among them"""
    if (k, n_keys, seed) not in _lists:
        rng = np.random.default_rng(seed)
        keys = np.unique(QM.canonical_np(rng.integers(0, 1 << (2 * k), size=3 * n_keys, dtype=np.uint64), k))
        keys = np.sort(rng.permutation(keys)[:n_keys])
        counts = rng.integers(1, 200, size=len(keys), dtype=np.uint32)
        counts[::7] = 0
        counts[1::7] = 0xFFFFFFFF
        _lists[(k, n_keys, seed)] = (keys, counts)
    return _lists[(k, n_keys, seed)]


def some_words(keys, k, n, seed, rate):
    """n canonical words, about `rate` of them words of the list (rate 1: all, 0: none)"""
    rng = np.random.default_rng(seed)
    cand = QM.canonical_np(rng.integers(0, 1 << (2 * k), size=2 * n + 64, dtype=np.uint64), k)
    absent = np.resize(cand[~np.isin(cand, keys)], n)
    present = keys[rng.integers(0, len(keys), size=n)]
    return np.where(rng.random(n) < rate, present, absent) if 0 < rate < 1 else (present if rate >= 1 else absent)


def ordinals_of(runs, first=0):
    """runs[s] words for sequence first + s"""
    return np.repeat(np.arange(len(runs), dtype=np.uint64) + np.uint64(first), runs)


def raw_of(ords, seed=9):
    """ordinal << 33 | position << 1 | strand, the low 33 bits anything"""
    rng = np.random.default_rng(seed)
    return (np.asarray(ords, dtype=np.uint64) << np.uint64(33)) | rng.integers(0, 1 << 33, size=len(ords), dtype=np.uint64)


def check(ctx, ix, keys, counts, k, words, runs, first=0, n_mm=0, pm_3=0, lo=1, hi=0xFFFFFFFF):
    ords = ordinals_of(runs, first)
    assert len(ords) == len(words)
    dw, dr = dev(words), dev(raw_of(ords))
    got = ctx.query_profile_words(ix, dw.data_ptr(), dr.data_ptr(), len(words), first, len(runs), n_mm, pm_3, lo, hi)
    want = SP.profile_words(keys, counts, words, ords.astype(np.int64), len(runs), k, n_mm, pm_3, lo, hi, first)
    rows = np.stack([got["n_words"], got["n_hits"], got["sum"]], axis=1) if len(runs) else np.zeros((0, 3), dtype=np.uint64)
    assert np.array_equal(rows, want), (runs[:8], np.flatnonzero((rows != want).any(axis=1))[:8], rows[:4], want[:4])
    return want


def run_shapes(T, W):
    """the lists of run lengths, by name"""
    rng = np.random.default_rng(77)
    return {
        "one-word": [1],
        "T+1-of-one": [1] * (T + 1),
        "one-of-6T+1": [6 * T + 1],
        "tile-edge": [T, T, 1],
        "across-tile-edge": [T - 1, 2, T - 1, 3],
        "round-edge": [W, W, W - 1, 1, 2 * W],
        "wave-edge": [WAVE, WAVE, 2 * WAVE, WAVE - 1, 1, WAVE + 1, WAVE - 1],
        "lanes-0-and-63": [WAVE - 1, 1, 1, WAVE - 2, 1, 1, WAVE - 1, 2, WAVE - 2, 1],
        "empty-between": [5] + [0] * (T + 3) + [7],
        "empty-first-and-last": [0, 0, 3, 0, T + 3, 0, 0],
        "reads": [100] * 45,
        "mixed": [int(x) for x in rng.choice([0, 1, 2, 3, 60, 64, 65, 300, 1000], size=40)],
    }


SHAPES = list(run_shapes(2048, 256))


def test_no_words_and_no_sequences(ctx):
    keys, counts = the_list(25, 3000, 1)
    ix = ctx.upload(make_records(keys, counts), 25).query_index()
    for n_mm in (0, 1):
        assert len(ctx.query_profile_words(ix, 0, 0, 0, 0, 0, n_mm)) == 0
        got = ctx.query_profile_words(ix, 0, 0, 0, 5, 3, n_mm)
        assert got.tobytes() == bytes(72)
    ix.free()


@pytest.mark.parametrize("shape", SHAPES)
def test_runs_without_mismatches(ctx, T, W, shape):
    k = 25
    keys, counts = the_list(k, 3000, 1)
    runs = run_shapes(T, W)[shape]
    n = sum(runs)
    ix = ctx.upload(make_records(keys, counts), k).query_index()
    want = check(ctx, ix, keys, counts, k, some_words(keys, k, n, 2, 0.5), runs, first=12345)
    if n > 100:
        assert want[:, 1].sum() > n // 4 and int(want[:, 2].max()) >= 0xFFFFFFFF
    # all hit: every word in the list and every value allowed (stored zeros are found); none hit: no word in the list
    want = check(ctx, ix, keys, counts, k, some_words(keys, k, n, 3, 1.0), runs, lo=0)
    assert (want[:, 0] == want[:, 1]).all()
    want = check(ctx, ix, keys, counts, k, some_words(keys, k, n, 4, 0.0), runs, lo=0)
    assert not want[:, 1].any() and not want[:, 2].any()
    ix.free()


@pytest.mark.parametrize("shape", ["one-word", "one-of-6T+1", "across-tile-edge", "lanes-0-and-63", "empty-between", "reads"])
@pytest.mark.parametrize("mm", [(1, 0), (2, 1)], ids=["mm1", "mm2-p1"])
def test_runs_with_mismatches(ctx, T, W, shape, mm):
    k = 9
    keys, counts = the_list(k, 40_000, 3)  # a third of the canonical 9-mers: variants do hit
    runs = run_shapes(T, W)[shape]
    n = sum(runs)
    ix = ctx.upload(make_records(keys, counts), k).query_index()
    want = check(ctx, ix, keys, counts, k, some_words(keys, k, n, 5, 0.5), runs, first=7, n_mm=mm[0], pm_3=mm[1])
    assert n < 100 or want[:, 1].sum() > n // 2
    check(ctx, ix, keys, counts, k, some_words(keys, k, n, 6, 0.5), runs, n_mm=mm[0], pm_3=mm[1], lo=300, hi=0x7FFFFFFF)
    ix.free()


def test_value_bounds_and_absent_words_under_a_minimum_of_zero(ctx, T):
    k = 25
    keys = np.arange(10, 20, dtype=np.uint64)  # (canonical: far below their reverse complements)
    counts = np.array([0, 1, 4, 5, 6, 9, 10, 11, 0xFFFFFFFF, 0xFFFFFFFF], dtype=np.uint32)
    words = np.concatenate([keys, np.arange(30, 40, dtype=np.uint64)])  # every key once, ten absent words
    runs = [10, 10]
    ix = ctx.upload(make_records(keys, counts), k).query_index()
    for lo, hi, hits, total in ((5, 10, 4, 30), (6, 9, 2, 15), (4, 11, 6, 45), (0, 0xFFFFFFFF, 10, 36 + 10 + 2 * 0xFFFFFFFF), (0, 0, 1, 0), (1, 0xFFFFFFFF, 9, 46 + 2 * 0xFFFFFFFF)):
        want = check(ctx, ix, keys, counts, k, words, runs, lo=lo, hi=hi)
        assert want.tolist() == [[10, hits, total], [10, 0, 0]], (lo, hi, want)
    ix.free()
    # with mismatches found means a sum other than 0: absent words with no neighbour in the list never hit under lo = 0
    k = 9
    keys, counts = np.array([0], dtype=np.uint64), np.array([3], dtype=np.uint32)
    ix = ctx.upload(make_records(keys, counts), k).query_index()
    far = QM.canonical_np(np.array([0b010101010101010101, 0b011001100110011001], dtype=np.uint64), k)
    want = check(ctx, ix, keys, counts, k, np.concatenate([far, np.array([1], dtype=np.uint64)]), [3], n_mm=1, lo=0)
    assert want.tolist() == [[3, 1, 3]]
    ix.free()


def test_ordinals_that_descend_or_leave_the_range_are_refused(ctx, T):
    from genometester4_amd import capi
    k = 25
    keys, counts = the_list(k, 3000, 1)
    ix = ctx.upload(make_records(keys, counts), k).query_index()
    n = T + 70
    words = dev(some_words(keys, k, n, 8, 0.5))
    good = ordinals_of([n // 2, n - n // 2], first=4)
    cases = {"descends": good[::-1].copy(), "descends-at-a-wavefront": np.concatenate([good[:WAVE] + np.uint64(1), good[WAVE:]]),
             "below": np.concatenate([[np.uint64(3)], good[1:]]), "above": np.concatenate([good[:-1], [np.uint64(6)]]),
             "far-above": np.concatenate([good[:-1], [np.uint64((1 << 31) - 1)]])}
    for n_mm in (0, 1):
        for name, ords in cases.items():
            with pytest.raises(capi.Gt4HipError) as e:
                ctx.query_profile_words(ix, words.data_ptr(), dev(raw_of(ords)).data_ptr(), n, 4, 2, n_mm)
            assert e.value.code == EINVAL and "ordinals" in str(e.value), (name, n_mm)
        got = ctx.query_profile_words(ix, words.data_ptr(), dev(raw_of(good)).data_ptr(), n, 4, 2, n_mm)  # the context goes on
        assert got["n_words"].tolist() == [n // 2, n - n // 2]
    with pytest.raises(capi.Gt4HipError) as e:
        ctx.query_profile_words(ix, words.data_ptr(), dev(raw_of(good)).data_ptr(), n, 4, 0)
    assert e.value.code == EINVAL
    ix.free()


# ------------------------------------------------------------------ gt4hip_query_profile_text

FASTA = (b">one first\nACGTACGTTGCATGCANNACGTAC\nGTACCATG\n>\nAC\n>three\tx\nACGTNACGTACGGTTACAGT\nTTGACCATGACGT\n>s1\nAC\n>s2\nA\n>s3\n\n"
         b">long name with spaces\nGGGGGGGGGGGGCCCCACGTACGATCGATCGATTTAGCATGCAGGGGACACACAGTGT\nACGATCGATCAGCTAGCATCGATCGnnACGATCAGCAGCGACTACGAC\n>last\nACG")
FASTQ = (b"@r1 a\nACGTACGTTGCATGCANNACGTACGTACCATG\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n@r2\nAC\n+r2\nII\n@\nACGTNACGTACGGTTACAGTTTGACCATGACGT\n+\n"
         b"IIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n@r4\nGGGGGGGGGGGGCCCCACGTACGATCGATCGATTTAGCATGCAGGGGACACACAGTGT\n+\n"
         b"IIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n@r5\nACGATCGATCAGCTAGCATCG\n+\nIIIIIIIIIIIIIIIIIIIII\n")


def text_list(text, k, seed):
    """about half of the text's words with counts, and as many words it does not hold"""
    words = np.unique(np.array(index_model.read_locations(text, k)[0], dtype=np.uint64))
    rng = np.random.default_rng(seed)
    keep = words[rng.random(len(words)) < 0.6]
    other = QM.canonical_np(rng.integers(0, 1 << (2 * k), size=len(keep) + 4, dtype=np.uint64), k)
    keys = np.unique(np.concatenate([keep, other]))
    counts = rng.integers(1, 50, size=len(keys), dtype=np.uint32)
    counts[::5] = 0xFFFFFFFF
    return keys, counts


@pytest.mark.parametrize("mm", [(0, 0), (1, 1)], ids=["mm0", "mm1-p1"])
@pytest.mark.parametrize("kind", ["fasta", "fastq"])
def test_text_cut_at_every_byte_adds_up_to_the_whole(ctx, kind, mm):
    text = FASTA if kind == "fasta" else FASTQ
    k = 7 if mm[0] == 0 else 5
    keys, counts = text_list(text, k, 11)
    ix = ctx.upload(make_records(keys, counts), k).query_index()
    names, want = SP.profile_text(keys, counts, text, k, mm[0], mm[1], 1, 0xFFFFFFFE)
    subs = index_model.read_locations(text, k)[4]
    assert want[:, 1].any() and (want[:, 1] == 0).any() and (want[:, 0] == 0).any()
    for cut in range(len(text) + 1):
        got, got_subs = ctx.query_profile_text(ix, [text[:cut], text[cut:]], mm[0], mm[1], 1, 0xFFFFFFFE)
        rows = np.stack([got["n_words"], got["n_hits"], got["sum"]], axis=1)
        assert np.array_equal(rows, want), (cut, rows, want)
        assert got_subs == subs, cut
    got, _ = ctx.query_profile_text(ix, [text[i:i + 1] for i in range(len(text))], mm[0], mm[1], 1, 0xFFFFFFFE)  # a byte a piece
    assert np.array_equal(np.stack([got["n_words"], got["n_hits"], got["sum"]], axis=1), want)
    ix.free()


def test_more_sequences_than_the_first_capacity(ctx):
    """the binding sizes its array from *n_profiles and calls again"""
    k = 4
    text = b"".join(b">s%d\n%s\n" % (i, b"ACGTTGCA"[: i % 9]) for i in range(300))
    keys, counts = text_list(text, k, 12)
    ix = ctx.upload(make_records(keys, counts), k).query_index()
    _, want = SP.profile_text(keys, counts, text, k)
    got, _ = ctx.query_profile_text(ix, [text])
    assert len(got) == 300 and np.array_equal(np.stack([got["n_words"], got["n_hits"], got["sum"]], axis=1), want)
    ix.free()


def test_a_reader_error_passes_through(ctx):
    from genometester4_amd import capi
    k = 4
    bad = b"@r1\nACGTACGT\n+\nIIIIIIII\n@r2\nACGTAC\nIIIIII\n"  # no '+' line behind the second read
    keys, counts = text_list(FASTQ, k, 13)
    ix = ctx.upload(make_records(keys, counts), k).query_index()
    with pytest.raises(capi.Gt4HipError) as ref:
        ctx.text_to_words(bad, k)
    with pytest.raises(capi.Gt4HipError) as e:
        ctx.query_profile_text(ix, [bad])
    assert e.value.code == EFORMAT and (e.value.error_offset, e.value.kind) == (ref.value.error_offset, ref.value.kind)
    assert e.value.kind == capi.MAKER_ERR_PLUS
    cut = 30  # the error lies in the second piece: the offset counts from its start
    with pytest.raises(capi.Gt4HipError) as e:
        ctx.query_profile_text(ix, [bad[:cut], bad[cut:]])
    assert e.value.code == EFORMAT and e.value.error_offset == ref.value.error_offset - cut
    with pytest.raises(capi.Gt4HipError) as e:
        ctx.query_profile_text(ix, [b"ACGT\n"])
    assert e.value.code == EFORMAT and e.value.kind == capi.MAKER_ERR_START
    ix.free()


def test_last_ms_reports_the_kernels(ctx, T):
    k = 25
    keys, counts = the_list(k, 3000, 1)
    ix = ctx.upload(make_records(keys, counts), k).query_index()
    check(ctx, ix, keys, counts, k, some_words(keys, k, 3 * T, 2, 0.5), [T, 2 * T])
    assert 0 < ix.last_ms < 1000
    ix.free()
