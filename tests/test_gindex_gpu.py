"""The table step of a location index through the C ABI: gt4hip_sort_pairs (the radix sort of gt4hip_sort.hip with a
64-bit value riding along) and gt4hip_pairs_to_index (sorted pairs -> the k-mer section and the location section of a
GT4I file, reference src/glistmaker.c:425-574), against numpy and against the reference's own index files.

Sizes: 20,001 pairs are two full 8192-pair tiles of the scatter kernel and a partial third, so the chained scan over
tiles and the bounds of the last tile both take part; 8192 and 16,384 end with a full tile (one tile: no look-back at
all); the fold's tiles are 8192 words, the index kernels' 1024 records.
Word lengths: ceil (2k / 9) passes, so k = 2, 11 end in the scratch buffers (1 and 3 passes: copied back) and k = 9, 25,
32 in place (2, 6, 8 passes); k = 25 and 32 take 9-bit digits, k = 32 every bit of the word."""
import hashlib

import numpy as np
import pytest

import gindex_util as G
import index_model as IM

pytestmark = pytest.mark.gpu
GOLDEN, GOLDEN_FILES = G.load()

from genometester4_amd import capi  # noqa: E402

N = 20_001


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def on_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()


def back(t):
    return t.cpu().numpy().view(np.uint64)


def spread_keys(k, n_distinct, rng):
    """n_distinct different words of k bases that reach into the topmost digit"""
    bits = 2 * k
    if bits <= 10:
        keys = rng.permutation(1 << bits)[:n_distinct].astype(np.uint64)
    else:
        keys = np.unique(rng.integers(0, 1 << (bits - 1), size=2 * n_distinct, dtype=np.uint64))[:n_distinct]
        keys[n_distinct // 2:] |= np.uint64(1 << (bits - 1))  # half of them with the word's top bit set
    assert len(np.unique(keys)) == n_distinct
    return keys


@pytest.mark.parametrize("k,n", [pytest.param(k, N, id=str(k)) for k in (2, 9, 11, 25, 32)]
                         + [pytest.param(k, n, id="%d-%d" % (k, n)) for k in (9, 11) for n in (8192, 16384)])  # full last tiles: in place, copied back
def test_pair_sort_is_stable_with_sixteen_keys(ctx, k, n):
    """value = where the pair stood in the input: after a stable sort the values ascend within every word, and together
    with the words they are exactly numpy's stable argsort"""
    rng = np.random.default_rng(k)
    words = spread_keys(k, 16, rng)[rng.integers(0, 16, size=n)]
    values = np.arange(n, dtype=np.uint64)
    w, v = on_device(words), on_device(values)
    ctx.sort_pairs(w.data_ptr(), v.data_ptr(), n, k)
    order = np.argsort(words, kind="stable")
    assert back(w).tolist() == words[order].tolist()
    assert back(v).tolist() == order.tolist()


@pytest.mark.parametrize("k", [11, 32])
def test_pair_sort_of_mostly_distinct_words(ctx, k):
    rng = np.random.default_rng(100 + k)
    words = spread_keys(k, 15_000, rng)[rng.integers(0, 15_000, size=N)]
    values = rng.integers(0, 1 << 63, size=N, dtype=np.uint64) * np.uint64(2) + np.uint64(1)  # all 64 bits of a value travel
    w, v = on_device(words), on_device(values)
    ctx.sort_pairs(w.data_ptr(), v.data_ptr(), N, k)
    order = np.argsort(words, kind="stable")
    assert (back(w) == words[order]).all()
    assert (back(v) == values[order]).all()


@pytest.mark.parametrize("n", [0, 1])
def test_pair_sort_of_nothing_and_of_one(ctx, n):
    w, v = on_device([7] * max(n, 1)), on_device([9] * max(n, 1))
    ctx.sort_pairs(w.data_ptr(), v.data_ptr(), n, 16)
    assert back(w).tolist() == [7] * max(n, 1) and back(v).tolist() == [9] * max(n, 1)
    kmers, n_locations, locs = ctx.pairs_to_index(w.data_ptr(), v.data_ptr(), n, 16)
    assert kmers.tolist() == [[7, 0]] * n and n_locations == n and locs.tolist() == [9] * n


@pytest.mark.parametrize("n,k", [(N, 2), (N, 11), (N, 9), (0, 16), (1, 16)])
def test_word_sort_against_numpy(ctx, n, k):
    """gt4hip_sort_words sorts in place: after 1 and 3 passes (k = 2, 11) the words come back from the scratch, after 2
    (k = 9) they lie in place; nothing and one word are left as they are"""
    rng = np.random.default_rng(200 + k)
    words = rng.integers(0, 1 << (2 * k), size=max(n, 1), dtype=np.uint64)
    w = on_device(words)
    ctx.sort_words(w.data_ptr(), n, k)
    assert back(w).tolist() == (np.sort(words) if n else words).tolist()


def expected_index(words, values, lo, hi):
    order = np.argsort(words, kind="stable")
    keys, counts = np.unique(words, return_counts=True)
    keep = (counts >= lo) & (counts <= hi)
    kept = counts[keep].astype(np.uint64)
    starts = np.concatenate([[0], np.cumsum(kept)[:-1]]).astype(np.uint64) if len(kept) else np.zeros(0, dtype=np.uint64)
    return np.stack([keys[keep], starts], axis=1), int(kept.sum()), values[order]


@pytest.fixture(scope="module")
def folded_input():
    """3,000 distinct words (three tiles of the index kernels) with one to about forty occurrences, 20,001 pairs"""
    rng = np.random.default_rng(7)
    keys = spread_keys(25, 3000, rng)
    weights = rng.integers(1, 5, size=3000).astype(float)
    weights[::97] = 40
    words = keys[rng.choice(3000, size=N, p=weights / weights.sum())]
    words[:3000] = keys  # every word occurs
    return words, np.arange(N, dtype=np.uint64)


@pytest.mark.parametrize("lo,hi", [(1, 0xffffffff), (2, 0xffffffff), (1, 3), (2, 3), (1000, 2000)], ids=["all", "c2", "max3", "c2max3", "none"])
def test_fold_with_the_cut_offs(ctx, folded_input, lo, hi):
    """the k-mer section holds the words the cut-offs keep, and their starts count the kept words' locations only; the
    location section is never filtered (reference src/glistmaker.c:486, :568)"""
    words, values = folded_input
    w, v = on_device(words), on_device(values)
    kmers, n_locations, locs = ctx.pairs_to_index(w.data_ptr(), v.data_ptr(), N, 25, lo, hi)
    exp_kmers, exp_n, exp_locs = expected_index(words, values, lo, hi)
    assert len(exp_kmers) > 0 or lo == 1000
    assert kmers.tolist() == exp_kmers.tolist()
    assert n_locations == exp_n
    assert locs.tolist() == exp_locs.tolist()


@pytest.fixture(scope="module")
def two_million_words():
    """2 x 1024 x 1024 + 5 distinct words with one or two occurrences each: 2049 tiles of the index kernels, so the scan of
    the tiles' sums (k_index_scan: one workgroup, rounds of 1024 tiles) carries both sums over two rounds into a third of
    one tile"""
    rng = np.random.default_rng(2049)
    n = 2 * 1024 * 1024 + 5
    keys = rng.permutation(np.unique(rng.integers(0, 1 << 50, size=n + n // 4, dtype=np.uint64)))[:n]
    assert len(keys) == n
    words = np.concatenate([keys, keys[rng.random(n) < 0.5]])
    return words[rng.permutation(len(words))], np.arange(len(words), dtype=np.uint64)


@pytest.mark.parametrize("lo", [1, 2])
def test_fold_of_more_tiles_than_two_rounds_of_the_scan(ctx, two_million_words, lo):
    words, values = two_million_words
    w, v = on_device(words), on_device(values)
    kmers, n_locations, locs = ctx.pairs_to_index(w.data_ptr(), v.data_ptr(), len(words), 25, lo)
    exp_kmers, exp_n, exp_locs = IM.sections(words, values, lo)
    exp_kmers = np.array(exp_kmers, dtype=np.uint64).reshape(-1, 2)
    assert len(exp_kmers) > 1024 * 1024 // 2 and kmers.shape == exp_kmers.shape
    assert (kmers == exp_kmers).all()
    assert n_locations == exp_n
    assert (locs == exp_locs).all()


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=[c["id"] for c in GOLDEN["cases"]])
def test_table_step_gives_the_reference_s_sections(ctx, case):
    """the reference's own `glistmaker --index` files: the words and packed locations of the texts (tests/index_model.py, in
    text order) through gt4hip_pairs_to_index give the k-mer and the location section of the golden file, cut-offs
    included; header and file block around them come from the model, and the whole file is compared under the mask"""
    k = case["k"]

    def on_gpu(words, locs, lo, hi):
        w, v = on_device(words), on_device(locs)
        kmers, n_locations, sorted_locs = ctx.pairs_to_index(w.data_ptr(), v.data_ptr(), len(words), k, lo, hi)
        return kmers, n_locations, sorted_locs

    texts = [G.file_bytes(GOLDEN, n) for n in case["inputs"]]
    got = IM.masked(IM.index_bytes(texts, case["inputs"], k, case["lo"], case["hi"], table=on_gpu))
    assert len(got) == case["bytes"]
    if case["id"] in GOLDEN_FILES:
        want = IM.parse(GOLDEN_FILES[case["id"]])
        have = IM.parse(got)
        assert (have["n_kmers"], have["n_locations"]) == (want["n_kmers"], want["n_locations"])
        assert have["kmers"].tolist() == want["kmers"].tolist()
        assert have["locations"].tolist() == want["locations"].tolist()
    assert hashlib.sha256(got).hexdigest() == case["sha256"]


def test_bad_arguments_are_refused(ctx):
    w, v = on_device([1, 2]), on_device([3, 4])
    for args in ((w.data_ptr(), v.data_ptr(), 2, 0, 1, 5), (w.data_ptr(), v.data_ptr(), 2, 33, 1, 5), (w.data_ptr(), v.data_ptr(), 2, 16, 0, 5),
                 (w.data_ptr(), v.data_ptr(), 2, 16, 3, 2), (w.data_ptr(), None, 2, 16, 1, 5)):
        with pytest.raises(capi.Gt4HipError) as e:
            ctx.pairs_to_index(*args)
        assert e.value.code == capi.EINVAL


# ---- the reader with locations (gt4hip_text_to_locations): words, raw locations and subsequence records against the model

SHORT_FASTA = (b">a first\nACGTTGCA\nNNacgu\r\n>short\nAC\n>\n\n>mid ACGT>line\nGGGTTTAAACCC>x\nACGTACGTAC"
               b"\n>two lines\nACGTAC\nGTTGCA\n>no end\nTTGACCA")
SHORT_FASTQ = b"@r1 x\nACGTTGCAAC\n+\nII@I+IIIII\n@r2\nNNACG\n+r2\n+@III\n@r3\n\n+\n\n@r4\nGATTACAGATT\n+\nIIIIIIIIIII\n"


def model_of(text, k):
    words, ords, poss, dirs, subs = IM.read_locations(text, k)
    raw = [(o << 33) | (p << 1) | d for o, p, d in zip(ords, poss, dirs)]
    return words, raw, subs, max(poss) if poss else 0


def check_pieces(ctx, text, k, cuts, want):
    pieces = [text[a:b] for a, b in zip([0] + list(cuts), list(cuts) + [len(text)])]
    words, raw, subs, max_pos = ctx.text_to_locations(pieces, k)
    assert words.tolist() == want[0], cuts
    assert raw.tolist() == want[1], cuts
    assert subs == want[2], cuts
    assert max_pos == want[3], cuts


@pytest.mark.parametrize("name,text,k", [("fasta", SHORT_FASTA, 3), ("fastq", SHORT_FASTQ, 4)])
def test_reader_locations_with_the_text_cut_at_every_offset(ctx, name, text, k):
    """two pieces, the cut at every offset of the text (0 and the end included: an empty piece): names, sequences, a word
    and a line break are all cut once, and every carry of the locations travels"""
    want = model_of(text, k)
    assert len(want[0]) > 10 and len(want[2]) >= 4
    for cut in range(len(text) + 1):
        check_pieces(ctx, text, k, [cut], want)


@pytest.fixture(scope="module")
def ten_kb():
    """about 10 kB: a sequence that covers the first tile boundary, a name of 700 bytes, short sequences, no final newline"""
    t = G.random_bases(5, 9000)
    text = (">first\n" + "".join(t[j:j + 60] + "\n" for j in range(0, 5000, 60)) + ">" + "long name " * 70 + "\n" + t[5000:5100] + "\n"
            + "".join(">s%d\n%s\n" % (j, t[5100 + 30 * j:5130 + 30 * j]) for j in range(100)) + ">last\n" + t[8100:9000]).encode()
    assert 10_000 < len(text) < 12_000
    return text, model_of(text, 11)


@pytest.mark.parametrize("where", ["4095", "4096", "4097", "mid-name", "mid-sequence", "three pieces"])
def test_reader_locations_of_ten_kilobytes_cut_around_a_tile(ctx, ten_kb, where):
    text, want = ten_kb
    name_at = text.index(b"long name") + 300
    cuts = {"mid-name": [name_at], "mid-sequence": [2000], "three pieces": [4097, name_at]}.get(where) or [int(where)]
    if where == "4095":
        check_pieces(ctx, text, 11, [], want)  # (and whole)
    check_pieces(ctx, text, 11, cuts, want)


def test_reader_locations_of_a_text_ended_by_a_nul(ctx):
    """a NUL is the reference's end of file: the open sequence ends there"""
    text = b">a\nACGTACGT\nAC\0GTTT\n>b\nAAAA\n"
    words, raw, subs, _ = ctx.text_to_locations([text[:7], text[7:]], 3)
    want = model_of(text, 3)
    assert (words.tolist(), raw.tolist(), subs) == want[:3]


def test_packed_locations_and_bit_sizes_of_two_files(ctx):
    """raw locations -> location words with the bit sizes of the model, file number in front (gt4hip_pack_locations)"""
    texts = [SHORT_FASTA, SHORT_FASTQ]
    words, locs, (fb, sb, pb), _ = IM.pairs(texts, 3)
    got = []
    for f, t in enumerate(texts):
        _, raw, _, _ = ctx.text_to_locations([t], 3)
        d = on_device(raw)
        ctx.pack_locations(d.data_ptr(), len(raw), f, sb, pb)
        got += back(d).tolist()
    assert got == locs
    d = on_device([1])
    for bits in ((0, 5), (5, 0), (31, 32), (5, 33)):
        with pytest.raises(capi.Gt4HipError) as e:
            ctx.pack_locations(d.data_ptr(), 1, 0, *bits)
        assert e.value.code == capi.EINVAL
    with pytest.raises(capi.Gt4HipError):
        ctx.pack_locations(d.data_ptr(), 1, 4, 30, 32)  # file 4 needs three bits: 3 + 30 + 32 + 1 > 64
