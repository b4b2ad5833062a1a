"""gt4hip_text_to_words / gt4hip_text_to_list (gt4hip_maker.hip) through the C ABI against tests/maker_model.py, on
texts sized by the kernels' tile of text (T bytes) and the emit stage's tile of codes: the places where a carry between
tiles, a halo or a compaction offset can go wrong."""
import numpy as np
import pytest

import gmaker_util as U
import maker_model as M

pytestmark = pytest.mark.gpu

from genometester4_amd import capi  # noqa: E402

RNG = np.random.default_rng(99)


def bases(n, rng=RNG):
    return bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)])


def fasta(n_bytes, line=61, rng=RNG):
    """a FastA text of exactly n_bytes: a name, then lines of `line` bases"""
    out = bytearray(b">s\n")
    while len(out) < n_bytes:
        out += bases(line, rng) + b"\n"
    return bytes(out[:n_bytes])


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def T(ctx):
    """bytes of text per tile of the kernels"""
    return ctx.get_counter("maker_text_tile")


@pytest.fixture(scope="module")
def E(ctx):
    """codes per tile of the emit stage"""
    return ctx.get_counter("maker_code_tile")


def check(ctx, text, k, flags=0):
    exp, err = M.read_words(text, k, canonize=not (flags & capi.MAKER_FORWARD_ONLY))
    assert err is None
    got, carry = ctx.text_to_words(text, k, flags)
    assert got.tolist() == exp
    return carry


@pytest.mark.parametrize("tiles,more", [(1, -1), (1, 0), (1, 1), (3, 17)], ids=["T-1", "T", "T+1", "3T+17"])
@pytest.mark.parametrize("k", [1, 16, 25, 32])
def test_text_lengths_around_the_tile(ctx, T, tiles, more, k):
    check(ctx, fasta(tiles * T + more), k)


def test_text_to_list_is_the_model_s_list(ctx, T):
    text = fasta(3 * T + 17)
    for k in (5, 25, 32):
        keys, counts = M.fold(M.read_words(text, k)[0])
        got = ctx.text_to_list(text, k).download()
        assert got["key"].tolist() == keys.tolist() and got["count"].tolist() == counts.tolist()


@pytest.mark.parametrize("k", [2, 16, 32])
def test_word_straddles_a_tile_edge_with_the_newline_on_the_edge(ctx, T, k):
    for nl_at in (T - 1, T, 2 * T - 1):  # the '\n' as the last byte of a tile and as the first of the next
        head = b">s\n"
        text = head + bases(nl_at - len(head)) + b"\n" + bases(2 * T)
        assert text[nl_at] == 10
        check(ctx, text, k)


@pytest.mark.parametrize("tiles,more", [(1, -1), (1, 0), (2, -1), (2, 0)], ids=["T-1", "T", "2T-1", "2T"])
def test_reset_as_the_last_and_the_first_byte_of_a_tile(ctx, T, E, tiles, more):
    at = tiles * T + more
    text = bytearray(fasta(3 * T, line=T))  # (long lines: the byte replaced is a base)
    text[at] = ord("N")
    check(ctx, bytes(text), 16)
    # the same position in code space: no line breaks, so byte i of the sequence is code i - 3
    flat = bytearray(b">s\n" + bases(3 * E))
    flat[3 + tiles * E + more] = ord("-")
    check(ctx, bytes(flat), 31)


def test_name_longer_than_a_tile(ctx, T):
    # begins in tile 0, covers tile 1 whole, ends in tile 2; holds '>' and bases that must not be read
    name = b">" + (b"ACGT>ACGTAC " * T)[:2 * T + 100] + b"\n"
    text = b">a\n" + bases(T - 200) + b"\n" + name + bases(300) + b"\n>b\n" + bases(50)
    assert len(text) > 3 * T
    check(ctx, text, 16)
    check(ctx, b">a\n" + bases(T - 200) + name + bases(300), 16)  # the name starts in mid-line


def test_fastq_record_over_four_tiles(ctx, T):
    recs = bytearray()
    for r in range(3):
        recs += b"@read %d " % r + b"n" * (T - 50) + b"\n" + bases(T + 13) + b"\n+" + b"p" * T + b"\n" + b"@>+I" * (T // 4 + 5) + b"\n"
    check(ctx, bytes(recs), 25)
    check(ctx, bytes(recs[:-1]), 25)  # no final newline


@pytest.mark.parametrize("k", [1, 5, 32])
def test_runs_of_k_minus_one_k_and_k_plus_one(ctx, k):
    text = b">s\n" + b"N".join(bases(n) for n in (k - 1, k, k + 1, k - 1, k + 1, k) if n) + b"\n"
    check(ctx, text, k)
    check(ctx, text, k, capi.MAKER_FORWARD_ONLY)


@pytest.mark.parametrize("k", [1, 32])
def test_all_t_run_at_full_width(ctx, k):
    text = b">s\n" + b"T" * 100 + b"\n" + b"A" * 40 + b"\n"
    check(ctx, text, k)
    check(ctx, text, k, capi.MAKER_FORWARD_ONLY)


def test_nul_in_mid_text_ends_it(ctx, T):
    text = bytearray(fasta(2 * T + 500))
    text[T + 77] = 0
    carry = check(ctx, bytes(text), 16)
    assert carry.ended == 1
    text = b"@r\n" + bases(40) + b"\n+\n" + b"I" * 40 + b"\n\x00@r2\n" + bases(40)
    assert check(ctx, text, 16).ended == 1


def test_text_without_a_word(ctx):
    for text in (b">only a name", b">s\nACGTACGTAC\n>t\nACGTANACGTA\n", b"", b"\x00>s\nACGTACGTACGTACGTACGT\n", b"@r\nACGT\n+\nIIII\n"):
        got, _ = ctx.text_to_words(text, 11)
        assert len(got) == 0
        assert ctx.text_to_list(text, 11).n_words == 0


def test_forward_only(ctx, T):
    text = fasta(T + 300) + b">x\nacgtuUACGN" + bases(70)
    check(ctx, text, 7, capi.MAKER_FORWARD_ONLY)
    check(ctx, text, 32, capi.MAKER_FORWARD_ONLY)


def test_text_in_device_memory(ctx, T):
    """TEXT_ON_DEVICE: the call reads the text where it lies (here: in the block of a list), first byte included"""
    from genometester4_amd.listio import RECORD_DTYPE
    for text in (fasta(2 * T + 333), b"@r\n" + bases(T + 5) + b"\n+\n" + b"I" * (T + 5) + b"\n", b"ACGT\n>x\nACGT\n"):
        block = ctx.upload(np.frombuffer(text + bytes(-len(text) % 12), dtype=RECORD_DTYPE), 16)
        exp, err = M.read_words(text, 16)
        if err is None:
            got, _ = ctx.text_to_words(block.device_ptr, 16, capi.MAKER_TEXT_ON_DEVICE, n_bytes=len(text))
            assert got.tolist() == exp
        else:
            with pytest.raises(capi.Gt4HipError) as e:
                ctx.text_to_words(block.device_ptr, 16, capi.MAKER_TEXT_ON_DEVICE, n_bytes=len(text))
            assert (e.value.code, e.value.kind, e.value.error_offset) == (capi.EFORMAT,) + err
        with pytest.raises(capi.Gt4HipError) as e:  # not 16-byte aligned
            ctx.text_to_words(block.device_ptr + 4, 16, capi.MAKER_TEXT_ON_DEVICE, n_bytes=8)
        assert e.value.code == capi.EINVAL
        block.free()


def test_pieces_with_a_carry_give_the_words_of_the_whole(ctx):
    """cuts inside a name, inside a quality line, k - 1 bases before a line end, behind a '\\n'"""
    k = 16
    fa = b">first name here\n" + bases(70) + b"\n" + bases(70) + b"\n>second>name\n" + bases(90) + b"\n"
    fq = b"@r1 name\n" + bases(60) + b"\n+\n" + b"@" + b"I" * 59 + b"\n@r2\n" + bases(60) + b"\n+r2\n" + b"+" * 60 + b"\n"
    for text, cuts in ((fa, (5, 17 + 70 - (k - 1), 17 + 71, 17 + 142 + 4, len(fa) - 1)), (fq, (4, 9 + 61 + 2 + 10, 9 + 60 - (k - 1), 9 + 61, 9 + 61 + 2, len(fq) - 1))):
        exp, err = M.read_words(text, k)
        assert err is None
        for cut in cuts:
            a, carry = ctx.text_to_words(text[:cut], k)
            b, end = ctx.text_to_words(text[cut:], k, carry=carry)
            assert a.tolist() + b.tolist() == exp, cut
            assert end.file_type == (1 if text is fa else 2)  # GT4HIP_MAKER_FASTA / _FASTQ


def test_error_offsets(ctx, T):
    bad = {
        b"ACGT\n>x\nACGT\n": (capi.MAKER_ERR_START, 0),
        b"@r1\n" + bases(T) + b"\n" + b"I" * T + b"\n@r2\nACGT\n+\nIIII\n": (capi.MAKER_ERR_PLUS, 4 + T + 1),
        b"@r1\nACGT\n+\nIIII\n" + b"r2\nACGT\n+\nIIII\n": (capi.MAKER_ERR_AT, 16),
        b"@r1\nACGT\n+\nIIII\n@r2\nACGT\nX\nIIII\n@r3\nACGT\nIIII\n": (capi.MAKER_ERR_PLUS, 25),  # the first of two
    }
    for text, (kind, at) in bad.items():
        assert M.read_words(text, 3)[1] == (kind, at)
        with pytest.raises(capi.Gt4HipError) as e:
            ctx.text_to_words(text, 3)
        assert (e.value.code, e.value.kind, e.value.error_offset) == (capi.EFORMAT, kind, at)
        with pytest.raises(capi.Gt4HipError) as e:
            ctx.text_to_list(text, 3)
        assert e.value.code == capi.EFORMAT
    # the end of the file behind a sequence line and inside a '+' line: the whole-text entry point reports it
    for text in (b"@r\nACGT\n", b"@r\nACGT\n+abc"):
        assert M.read_words(text, 3)[1] is not None
        with pytest.raises(capi.Gt4HipError) as e:
            ctx.text_to_list(text, 3)
        assert e.value.code == capi.EFORMAT
    assert capi.lib().gt4hip_strerror(capi.EFORMAT) == b"malformed sequence text"
