"""gt4hip_gmer.hip at the library level through capi, against numpy (searchsorted + bincount) for the counting kernel and
against tests/gmer_model.py (held to the reference in tests/test_gmer_model.py) for the text entry point."""
import numpy as np
import pytest

import gmer_model as M
import gmer_util as U

pytestmark = pytest.mark.gpu

CASES = U.load_cases()
NS = (0, 1, 63, 64, 65, 255, 257, 70_001)


@pytest.fixture(scope="module")
def ctx():
    from genometester4_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()


def _canonical(w, k):
    w = np.asarray(w, dtype=np.uint64)
    x, r = ~w, np.zeros_like(w)
    for _ in range(k):
        r = (r << np.uint64(2)) | (x & np.uint64(3))
        x = x >> np.uint64(2)
    return np.minimum(w, r)


def _db_words(rng, n, k):
    """n words of k bases, either strand, no canonical word twice"""
    top = (1 << (2 * k)) - 1
    got = np.zeros(0, dtype=np.uint64)
    while True:
        w = rng.integers(0, top, size=2 * n + 16, dtype=np.uint64, endpoint=True)
        got = np.concatenate([got, w])
        _, first = np.unique(_canonical(got, k), return_index=True)
        got = got[np.sort(first)]
        if len(got) >= n:
            return got[:n]


def _expect(db_words, k, words):
    """(counts per k-mer, hits, GC term) by searchsorted + bincount"""
    canon = _canonical(db_words, k)
    order = np.argsort(canon, kind="stable")
    srt = canon[order]
    words = np.asarray(words, dtype=np.uint64)
    at = np.searchsorted(srt, words)
    at[at == len(srt)] = 0
    hit = srt[at] == words if len(words) else np.zeros(0, dtype=bool)
    counts = np.bincount(order[at[hit]], minlength=len(db_words)).astype(np.uint64)
    gc = int(((words[hit] ^ (words[hit] >> np.uint64(1))) & np.uint64(1)).sum())
    return counts, int(hit.sum()), gc


def _queries(rng, db_words, k, n, rate):
    """n words of which about `rate` are (canonical) database words"""
    canon = _canonical(db_words, k)
    cand = _canonical(rng.integers(0, (1 << (2 * k)) - 1, size=2 * n + 4096, dtype=np.uint64, endpoint=True), k)
    absent = cand[~np.isin(cand, canon)]
    assert len(absent)
    absent = np.resize(absent, n)
    present = canon[rng.integers(0, len(canon), size=n)]
    if rate >= 1:
        return present
    return np.where(rng.random(n) < rate, present, absent) if rate > 0 else absent


@pytest.mark.parametrize("k", (5, 25, 32))
@pytest.mark.parametrize("n_db", (1, 9, 5000))
def test_count_words_against_numpy(ctx, k, n_db):
    from genometester4_amd import capi
    if k == 5 and n_db == 5000:
        n_db = 500  # (there are 512 canonical 5-mers)
    rng = np.random.default_rng(1000 * k + n_db)
    dbw = _db_words(rng, n_db, k)
    db = ctx.gmer_db(dbw, k)
    try:
        assert db.n_kmers == n_db
        for rate in (0.0, 0.01, 1.0):
            for n in NS:
                q = _queries(rng, dbw, k, n, rate)
                counts, hits, gc = _expect(dbw, k, q)
                for flags in (0, capi.GMER_PLAIN_ATOMICS):
                    db.reset()
                    assert db.count_words(q, flags) == (hits, gc), (rate, n, flags)
                    assert np.array_equal(db.counts(), counts), (rate, n, flags)
                if n in (65, 70_001):  # device words
                    d = _dev(q)
                    db.reset()
                    assert db.count_words(d.data_ptr(), capi.GMER_ON_DEVICE, n) == (hits, gc)
                    assert np.array_equal(db.counts(), counts)
    finally:
        db.free()


def test_one_wavefront_on_one_kmer_and_on_64_kmers(ctx):
    from genometester4_amd import capi
    rng = np.random.default_rng(5)
    dbw = _db_words(rng, 200, 25)
    canon = _canonical(dbw, 25)
    db = ctx.gmer_db(dbw, 25)
    try:
        for q in (np.full(64, canon[17]), canon[:64], np.concatenate([np.full(64, canon[3]), canon[64:128], np.full(30, canon[3]), canon[5:9]]),
                  np.concatenate([np.full(63, canon[9]), canon[10:11]]), np.concatenate([[np.uint64(1)] * 40, np.full(24, canon[0])]).astype(np.uint64)):
            counts, hits, gc = _expect(dbw, 25, q)
            for flags in (0, capi.GMER_PLAIN_ATOMICS):
                db.reset()
                assert db.count_words(q, flags) == (hits, gc)
                assert np.array_equal(db.counts(), counts)
    finally:
        db.free()


def test_calls_accumulate_and_reset_clears(ctx):
    rng = np.random.default_rng(6)
    dbw = _db_words(rng, 9, 25)
    db = ctx.gmer_db(dbw, 25)
    try:
        a, b = _queries(rng, dbw, 25, 257, 1.0), _queries(rng, dbw, 25, 1000, 0.5)
        ca, cb = _expect(dbw, 25, a)[0], _expect(dbw, 25, b)[0]
        db.count_words(a)
        db.count_words(b)
        assert np.array_equal(db.counts(), ca + cb)
        assert np.array_equal(db.counts(3, 4), (ca + cb)[3:7])
        db.reset()
        assert not db.counts().any()
        db.count_words(b)
        assert np.array_equal(db.counts(), cb)
    finally:
        db.free()


def _revcomp(w, k):
    r = 0
    for _ in range(k):
        r, w = (r << 2) | (~w & 3), w >> 2
    return r


def test_duplicates_are_refused_and_leak_nothing(ctx):
    from genometester4_amd import capi
    w = int("00011011" * 2 + "00", 2)  # ACGTACGTA
    rc = _revcomp(w, 9)
    assert rc != w and int(_canonical(np.array([rc], dtype=np.uint64), 9)[0]) == min(w, rc)
    fwd = [int(x) for x in _db_words(np.random.default_rng(7), 60, 9) if min(int(x), _revcomp(int(x), 9)) != min(w, rc)][:50]
    ctx.gmer_db(np.array([0b00011011], dtype=np.uint64), 4).free()  # ACGT is its own reverse complement: one word, no duplicate
    free0 = None
    for rep in range(20):
        for words, pair in ((fwd[:20] + [fwd[3]], (3, 20)), ([w] + fwd[:5] + [rc], (0, 6)), ([fwd[0], fwd[0]], (0, 1)), ([rc, w], (0, 1))):
            with pytest.raises(capi.Gt4HipError) as e:
                ctx.gmer_db(np.array(words, dtype=np.uint64), 9)
            assert e.value.code == capi.EINVAL and ("%d and %d" % pair) in str(e.value), str(e.value)
        with pytest.raises(capi.Gt4HipError) as e:  # a word that does not fit 9 bases
            ctx.gmer_db(np.array([1 << 18], dtype=np.uint64), 9)
        assert e.value.code == capi.EINVAL
        if rep == 0:
            free0 = ctx.device_memory()[0]  # (the pool holds what the first round left)
    assert ctx.device_memory()[0] >= free0


def _whole_and_pieces(ctx, dbm, text, cuts):
    """the sums over the pieces of `text` cut at `cuts`, and the counters"""
    db = ctx.gmer_db(np.array([w for ws in dbm.words for w in ws], dtype=np.uint64), dbm.wordsize)
    try:
        total = dict(n_n=0, n_nucl=0, n_gc=0, n_words=0, n_hits=0, n_kmer_gc=0)
        carry, at = None, 0
        for end in list(cuts) + [len(text)]:
            st, carry = db.count_text(text[at:end], carry)
            for f in total:
                total[f] += getattr(st, f)
            at = end
        return total, [int(c) for c in db.counts()]
    finally:
        db.free()


@pytest.mark.parametrize("name,dbname", [("reads.fq", "db16.txt"), ("multi.fa", "db5.txt"), ("crlf.fa", "db25.txt"), ("nofinal.fa", "db32.txt")])
def test_count_text_equals_the_model(ctx, name, dbname):
    dbm, _ = M.parse_db(U.file_bytes(CASES, dbname))
    text = U.file_bytes(CASES, name)
    counts, st, err = M.count(dbm, [text])
    assert err is None
    assert _whole_and_pieces(ctx, dbm, text, []) == (st, counts)
    assert _whole_and_pieces(ctx, dbm, text, [len(text) // 3, len(text) // 3 + 1, 2 * len(text) // 3]) == (st, counts)


def test_count_text_cut_at_every_offset_of_a_fastq_record(ctx):
    dbm, _ = M.parse_db(U.file_bytes(CASES, "db16.txt"))
    text = U.file_bytes(CASES, "reads.fq")
    counts, st, err = M.count(dbm, [text])
    assert err is None and st["n_hits"] > 0 and st["n_n"] > 0
    start = text.index(b"@r2 ")
    end = text.index(b"@r3 ")
    db = ctx.gmer_db(np.array([w for ws in dbm.words for w in ws], dtype=np.uint64), 16)
    try:
        for cut in range(start, end + 1):
            db.reset()
            total = dict.fromkeys(st, 0)
            carry = None
            for piece in (text[:cut], text[cut:]):
                s, carry = db.count_text(piece, carry)
                for f in total:
                    total[f] += getattr(s, f)
            assert total == st, cut
            assert [int(c) for c in db.counts()] == counts, cut
    finally:
        db.free()


def test_count_text_generated_reads_and_a_nul(ctx):
    dbm, _ = M.parse_db(U.file_bytes(CASES, "dbbig.txt"))
    text = U.file_bytes(CASES, "big.fq")[:40_000]
    text = text[:text.rindex(b"@read")]
    counts, st, err = M.count(dbm, [text])
    assert err is None and st["n_hits"] > 1000
    assert _whole_and_pieces(ctx, dbm, text, [4096, 8191, 30_001]) == (st, counts)
    # a NUL ends the text: what lies behind it gives nothing, in the piece that holds it and in the pieces behind
    cut = text.index(b"\n@read40 ") + 1
    with_nul = text[:cut] + b"\0" + text[cut:]
    counts, st, err = M.count(dbm, [text[:cut]])
    assert _whole_and_pieces(ctx, dbm, with_nul, [cut + 100]) == (st, counts)
    assert _whole_and_pieces(ctx, dbm, with_nul, [cut - 7, cut + 1]) == (st, counts)


def test_count_text_errors_are_the_readers(ctx):
    from genometester4_amd import capi
    dbm, _ = M.parse_db(U.file_bytes(CASES, "db5.txt"))
    db = ctx.gmer_db(np.array([w for ws in dbm.words for w in ws], dtype=np.uint64), 5)
    try:
        for name, kind, at in (("bad_start.fa", capi.MAKER_ERR_START, 0), ("no_plus.fq", capi.MAKER_ERR_PLUS, 25)):
            with pytest.raises(capi.Gt4HipError) as e:
                db.count_text(U.file_bytes(CASES, name))
            assert (e.value.code, e.value.kind, e.value.error_offset) == (capi.EFORMAT, kind, at)
    finally:
        db.free()
