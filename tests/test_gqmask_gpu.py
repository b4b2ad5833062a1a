"""gt4hip_mask.hip at the library level through capi (Context.query_mask_text), against tests/mask_model.py (held to the
reference in tests/test_gqmask_model.py) and the goldens themselves, at the smallest shapes where the two kernels can go
wrong: a hit word slid base by base over the edges of a thread, a wavefront, a tile and two tiles of codes and of text, the
64-bit extract at every bit offset, covers that overlap, touch and leave one base, pieces cut at every offset.  The module's
context runs with option "poison": nothing may depend on what a pooled block held.

Per piece the test holds n_covered and back to the model exactly.  The sum "n_covered + back = covered bases" holds for a
text in one piece; over several pieces a base covered by a hit word of its own piece AND by one that ends in a later piece
is counted by both, so there the sum is held to be no less than the covered bases."""
import numpy as np
import pytest

import gqmask_util as U
import mask_model as MM
import query_model as QM
import reader_texts as RT
from genometester4_amd.listio import make_records

pytestmark = pytest.mark.gpu

EINVAL, EFORMAT = 1, 11
T = 4096


@pytest.fixture(scope="module")
def ctx():
    from genometester4_amd import capi
    c = capi.Context(0)
    c.set_option("poison", 1)
    assert c.get_counter("maker_text_tile") == T == c.get_counter("maker_code_tile")
    yield c
    c.close()


@pytest.fixture(scope="module")
def index_of(ctx):
    """the query index of (keys, counts, k), made once per module"""
    made = {}

    def get(keys, counts, k):
        key = (keys.tobytes(), counts.tobytes(), k)
        if key not in made:
            made[key] = ctx.upload(make_records(keys, counts), k).query_index()
        return made[key]
    yield get
    for ix in made.values():
        ix.free()


def pieces_of(text, cuts):
    edges = [0] + list(cuts) + [len(text)]
    return [text[s:e] for s, e in zip(edges[:-1], edges[1:])]


def check(ctx, ix, m, k, cuts, mm=0, pm=0, lo=1, hi=0xFFFFFFFF, soft=False, upto=None):
    """the text of the model's result `m` through the library in the pieces the cuts make, held to the model"""
    text = m.source if upto is None else m.source[:upto]
    got, recs = ctx.query_mask_text(ix, pieces_of(text, cuts), mm, pm, lo, hi, soft)
    want = m.text if upto is None else m.text[:upto]
    if got != want:
        at = next(i for i in range(len(want)) if got[i] != want[i])
        raise AssertionError((cuts, at, got[max(0, at - 40):at + 40], want[max(0, at - 40):at + 40]))
    backs = [r["back"] for r in recs]
    assert all(b <= k - 1 for b in backs), (cuts, backs)
    assert backs == m.backs(cuts), (cuts, backs, m.backs(cuts))
    assert [r["n_covered"] for r in recs] == m.own_covered(cuts), (cuts, recs)
    total = sum(r["n_covered"] for r in recs) + sum(backs)
    assert total >= m.counts[2] and (cuts or total == m.counts[2]), (cuts, total, m.counts)
    assert (sum(r["n_words"] for r in recs), sum(r["n_hits"] for r in recs)) == m.counts[:2], (cuts, recs, m.counts)
    return recs


def model(keys, counts, text, k, mm=0, pm=0, lo=1, hi=0xFFFFFFFF, soft=False):
    m = MM.mask_text(keys, counts, text, k, mm, pm, lo, hi, soft)
    m.source = text
    return m


# ------------------------------------------------------------------ the goldens

@pytest.mark.parametrize("case", U.COMPUTED, ids=lambda c: c["id"])
def test_golden_whole_cut_in_two_at_every_offset_and_a_byte_a_piece(ctx, index_of, case):
    lst, fname, mm, pm, lo, hi, soft = U.parse(case["argv"])
    keys, counts, k = U.keys_counts(lst)
    text = U.text_of(fname)
    m = model(keys, counts, text, k, mm, pm, lo, hi, soft)
    assert m.text.decode("latin-1") == case["stdout"] and list(m.counts) == case["counts"]  # (the golden itself is the expectation)
    ix = index_of(keys, counts, k)
    check(ctx, ix, m, k, [], mm, pm, lo, hi, soft)
    for cut in range(len(text) + 1):
        check(ctx, ix, m, k, [cut], mm, pm, lo, hi, soft)
    check(ctx, ix, m, k, list(range(1, len(text))), mm, pm, lo, hi, soft)


# ------------------------------------------------------------------ the edge sweep

N_CODES = 2 * T + T // 4 + 40
CODE_EDGES = (16, 1024, 4096, 8192)


def layout(codes: bytes, line):
    """(the sequence's bytes, code index -> byte offset in them): no line breaks, or a '\\n' behind every `line` bases"""
    if not line:
        return codes, lambda c: c
    return b"".join(codes[i:i + line] + b"\n" for i in range(0, len(codes), line)), lambda c: c + c // line


def slide_starts(k, line):
    """first-base code indices: k + 1 positions across every code edge; with line breaks also across the codes that stand at
    the byte edges, so that those fall inside the word"""
    edges = set(CODE_EDGES)
    if line:
        edges |= {e - e // (line + 1) for e in (1024, 4096, 8192)}
    return sorted({s for e in edges for s in range(e - k, e + 1) if s >= 0})


def background(n, seed, letters=b"CG"):
    return bytes(np.frombuffer(letters, dtype=np.uint8)[np.random.default_rng(seed).integers(0, len(letters), size=n)])


@pytest.mark.parametrize("line", [0, 60], ids=["no-breaks", "61-byte-lines"])
@pytest.mark.parametrize("k", [1, 16, 17, 32])
def test_one_hit_word_slid_over_the_edges(ctx, index_of, k, line):
    """the text goes in as two pieces, the name line and the sequence: without line breaks a code's index in the second
    piece is its byte offset there and a thread's first code is a multiple of 16; with 61-byte lines the threads' first codes
    take every residue, which walks k_mask_apply's 64-bit extract over every bit offset"""
    keys, counts = np.array([0], dtype=np.uint64), np.array([1], dtype=np.uint32)  # A...A, which no run of C and G holds
    ix = index_of(keys, counts, k)
    bg = background(N_CODES, k)
    head = b">s\n"
    for s in slide_starts(k, line):
        codes = bg[:s] + b"A" * k + bg[s + k:]
        body, at = layout(codes, line)
        text = head + body
        m = model(keys, counts, text, k)
        assert m.counts[1:] == (1, k) and m.text[len(head) + at(s)] == ord("N") and m.text[len(head) + at(s + k - 1)] == ord("N")
        recs = check(ctx, ix, m, k, [len(head)])
        assert recs[1]["n_covered"] == k


@pytest.mark.parametrize("line", [0, 60], ids=["no-breaks", "61-byte-lines"])
@pytest.mark.parametrize("k", [1, 16, 17, 32])
def test_two_hit_words_whose_covers_overlap_touch_and_leave_one_base(ctx, index_of, k, line):
    """A..AC and CA..A in a run of G: at distance k - 1 they share the C, at k they touch, at k + 1 one G stays between them
    (k = 1: two A in a run of C and G, one and two apart)"""
    if k == 1:
        keys, first, second, bg, dists = np.array([0], dtype=np.uint64), b"A", b"A", background(N_CODES, 5), (1, 2)
    else:
        keys, first, second, bg, dists = np.array([1, 1 << (2 * (k - 1))], dtype=np.uint64), b"A" * (k - 1) + b"C", b"C" + b"A" * (k - 1), b"G" * N_CODES, (k - 1, k, k + 1)
    counts = np.ones(len(keys), dtype=np.uint32)
    ix = index_of(keys, counts, k)
    head = b">s\n"
    for d in dists:
        for s in slide_starts(k, line):
            codes = bytearray(bg)
            codes[s:s + k] = first
            codes[s + d:s + d + k] = second
            body, at = layout(bytes(codes), line)
            m = model(keys, counts, head + body, k)
            assert m.counts[1:] == (2, min(d, k) + k), (d, s, m.counts)
            check(ctx, ix, m, k, [len(head)])
            if s in (CODE_EDGES[2] - k, CODE_EDGES[2] - 1):
                check(ctx, ix, m, k, [len(head), len(head) + at(s + d)])  # the second word begins a piece of its own


# ------------------------------------------------------------------ lists that hit everything and nothing

def all_words(k):
    keys = np.unique(QM.canonical_np(np.arange(4 ** k, dtype=np.uint64), k))
    return keys, np.arange(1, len(keys) + 1, dtype=np.uint32)


@pytest.mark.parametrize("kind", RT.KINDS)
def test_all_hit_list_over_the_reader_s_probes_at_the_edges(ctx, index_of, kind):
    """every base of every run of k and more changes, no byte of a name, a '+' or a quality line does"""
    k = RT.K
    keys, counts = all_words(k)
    ix = index_of(keys, counts, k)
    n = 0
    for edge in RT.EDGES.values():
        for pad_kind in RT.PAD_KINDS[kind]:
            for i, (at, text) in enumerate(RT.sweep(kind, edge, pad_kind)):
                if i % (1 if (edge == T and pad_kind == "sequence") else 9):
                    continue
                m = model(keys, counts, text, k)
                assert m.err is None and m.counts[0] == m.counts[1] > 0
                check(ctx, ix, m, k, [])
                check(ctx, ix, m, k, sorted([at, edge]))
                n += 1
    assert n > 60
    # the property, spelled out on the probe itself: what changed are bases of sequence lines, and every one of a run >= k
    text = RT.probe(kind)
    got, _ = ctx.query_mask_text(ix, [text], 0, 0, 1, 0xFFFFFFFF)
    words, last, bases, err = MM.read_bases(text, k)
    in_word = set()
    for e in last:
        in_word.update(bases[e - k + 1:e + 1])
    assert err is None and {i for i in range(len(text)) if got[i] != text[i]} == in_word and all(got[i] == ord("N") for i in in_word)


def test_no_hit_list_gives_the_text_back(ctx, index_of):
    k = RT.K
    keys, counts = np.array([0], dtype=np.uint64), np.array([0], dtype=np.uint32)  # a stored count of 0 is found and no hit under lo = 1
    ix = index_of(keys, counts, k)
    for kind in RT.KINDS:
        text = RT.padded(kind, "sequence", T - 7, RT.swept(kind, "sequence"), RT.tail(kind)) + b"AAAAAAAA\n" * (kind == "fasta")
        for soft in (False, True):
            got, recs = ctx.query_mask_text(ix, [text[:T + 3], text[T + 3:]], 0, 0, 1, 0xFFFFFFFF, soft)
            assert got == text and all(r["n_hits"] == r["n_covered"] == r["back"] == 0 for r in recs) and sum(r["n_words"] for r in recs) > 1000


def test_soft_against_hard_on_the_same_text(ctx, index_of):
    k = 9
    keys, counts, _ = U.keys_counts("K9")
    ix = index_of(keys, counts, k)
    text = U.text_of("small.fa") * 40  # lower case, U and u among the covered bases; more than two tiles
    assert len(text) > 2 * T
    hard, rh = ctx.query_mask_text(ix, [text], 0, 0, 1, 0xFFFFFFFF, False)
    soft, rs = ctx.query_mask_text(ix, [text], 0, 0, 1, 0xFFFFFFFF, True)
    other, _ = ctx.query_mask_text(ix, [text], 0, 0, 1, 0xFFFFFFFF, False, b"x")
    assert rh == rs and rh[0]["n_covered"] > 1000
    changed = [i for i in range(len(text)) if hard[i] != text[i]]
    assert len(changed) == rh[0]["n_covered"]  # (no covered base is an N already)
    assert all(soft[i] == text[i] | 0x20 for i in changed) and all(soft[i] == text[i] for i in set(range(len(text))) - set(changed))
    assert all(other[i] == ord("x") for i in changed) and all(other[i] == text[i] for i in set(range(len(text))) - set(changed))
    assert any(text[i] == ord("U") and soft[i] == ord("u") for i in changed) and any(text[i] == ord("a") and soft[i] == ord("a") for i in changed)
    m = model(keys, counts, text, k)
    assert hard == m.text


@pytest.mark.parametrize("nul", [1023, 4096, 2 * T + 100])
def test_bytes_behind_a_nul_come_back_untouched(ctx, index_of, nul):
    k = 9
    keys, counts, _ = U.keys_counts("ALL9")
    ix = index_of(keys, counts, k)
    base = U.text_of("small.fa") * 40
    text = base[:nul] + b"\0" + base[nul + 1:2 * T + 300]
    m = model(keys, counts, text, k)
    assert m.text[nul:] == text[nul:] and m.counts[2] > nul // 4
    check(ctx, ix, m, k, [])
    check(ctx, ix, m, k, [nul])
    check(ctx, ix, m, k, [nul + 1, nul + 500])  # pieces behind the end of the text are copied
    got, recs = ctx.query_mask_text(ix, [b"\0" + base[:100]], 0, 0, 1, 0xFFFFFFFF)  # a NUL first: an empty file
    assert got == b"\0" + base[:100] and recs[0] == {"n_words": 0, "n_hits": 0, "n_covered": 0, "back": 0}


def test_malformed_text_raises_as_text_to_words_does(ctx, index_of):
    from genometester4_amd import capi
    keys, counts, k = U.keys_counts("K9")
    ix = index_of(keys, counts, k)
    for case in U.MALFORMED:
        lst, fname, mm, pm, lo, hi, soft = U.parse(case["argv"])
        bad = U.text_of(fname)
        with pytest.raises(capi.Gt4HipError) as ref:
            ctx.text_to_words(bad, k)
        with pytest.raises(capi.Gt4HipError) as e:
            ctx.query_mask_text(ix, [bad], mm, pm, lo, hi, soft)
        assert e.value.code == EFORMAT and (e.value.error_offset, e.value.kind) == (ref.value.error_offset, ref.value.kind) and e.value.kind == capi.MAKER_ERR_PLUS
        assert ref.value.error_offset == len(case["stdout"])
        cut = 30
        with pytest.raises(capi.Gt4HipError) as e:
            ctx.query_mask_text(ix, [bad[:cut], bad[cut:]], mm, pm, lo, hi, soft)
        assert e.value.code == EFORMAT and e.value.error_offset == ref.value.error_offset - cut
        # the bytes in front of the offending byte, as the command line runs them again: the golden
        m = model(keys, counts, bad, k, mm, pm, lo, hi, soft)
        assert m.text[:m.err[1]].decode("latin-1") == case["stdout"]
        check(ctx, ix, m, k, [], mm, pm, lo, hi, soft, upto=m.err[1])
    with pytest.raises(capi.Gt4HipError) as e:
        ctx.query_mask_text(ix, [b"ACGT\n"])
    assert e.value.code == EFORMAT and e.value.kind == capi.MAKER_ERR_START


def test_a_wrong_argument_is_einval_without_a_launch(ctx, index_of):
    import ctypes as C
    from genometester4_amd import capi
    keys, counts, k = U.keys_counts("K9")
    ix = index_of(keys, counts, k)
    L = capi.lib()
    text = b">s\nACGTACGTACGTACGT\n"
    buf, got = C.create_string_buffer(text, len(text)), C.create_string_buffer(len(text))
    prm, out, piece, err = capi.QueryParams(0, 0, 1), capi.MakerCarry(), capi.MaskPiece(), C.c_uint64()

    def call(h=ctx.h, q=ix.h, t=buf, flags=0, p=prm, o=out, masked=got, pc=piece, carry=None):
        return L.gt4hip_query_mask_text(h, q, t, len(text), flags, C.byref(p) if p is not None else None, 1, 0xFFFFFFFF, ord("N"), carry,
                                        C.byref(o) if o is not None else None, masked, C.byref(pc) if pc is not None else None, C.byref(err))
    ctx.query_mask_text(ix, [text])
    capped = ctx.get_counter("grid_capped")
    ms = ix.last_ms
    assert ms > 0
    assert call() == 0 and got.raw == ctx.query_mask_text(ix, [text])[0]
    for kw in (dict(h=None), dict(q=None), dict(t=None), dict(p=None), dict(o=None), dict(masked=None), dict(pc=None), dict(flags=1), dict(flags=8), dict(flags=16)):
        assert call(**kw) == EINVAL, kw
    assert call(p=capi.QueryParams(k, 1, 1)) == EINVAL and "gt4hip_query_mask_text" in L.gt4hip_last_error(ctx.h).decode()
    bad = capi.MakerCarry()
    bad.file_type = 7
    assert call(carry=C.byref(bad)) == EINVAL
    assert call(flags=capi.MAKER_TEXT_ON_DEVICE, masked=C.c_void_p(8), t=C.c_void_p(4096)) == EINVAL  # device memory that is not 16-byte aligned
    assert ctx.get_counter("grid_capped") == capped
    assert call() == 0  # the context goes on


def test_text_and_masked_text_on_the_device(ctx, index_of):
    import ctypes as C
    import torch
    from genometester4_amd import capi
    keys, counts, k = U.keys_counts("K9")
    ix = index_of(keys, counts, k)
    text = U.text_of("small.fa") * 12
    m = model(keys, counts, text, k)
    d_text = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    d_out = torch.full((len(text) + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    prm, out, piece, err = capi.QueryParams(0, 0, 1), capi.MakerCarry(), capi.MaskPiece(), C.c_uint64()
    rc = capi.lib().gt4hip_query_mask_text(ctx.h, ix.h, C.c_void_p(d_text.data_ptr()), len(text), capi.MAKER_TEXT_ON_DEVICE, C.byref(prm), 1, 0xFFFFFFFF, ord("N"), None,
                                           C.byref(out), C.c_void_p(d_out.data_ptr()), C.byref(piece), C.byref(err))
    assert rc == 0, capi.lib().gt4hip_last_error(ctx.h)
    got = d_out.cpu().numpy().tobytes()
    assert got[:len(text)] == m.text and got[len(text):] == b"\x5a" * 64
    assert (piece.n_words, piece.n_hits, piece.n_covered, piece.back) == (*m.counts, 0)
    assert 0 < ix.last_ms < 1000
