"""tests/reader_texts.py held to what it promises, on the CPU: a GPU test that draws its texts from there cannot pass by
covering nothing.  The models are those of tests/maker_model.py and tests/index_model.py."""
import re

import numpy as np
import pytest

import index_model as IM
import maker_model as M
import reader_texts as R

SWEEPS = [(kind, edge, pad) for kind in R.KINDS for edge in R.EDGES for pad in R.PAD_KINDS[kind]]


def test_geometry_is_the_sources():
    host = open(R.CSRC + "/gt4hip_host.h").read()
    assert R.T == int(re.search(r"#define GT4HIP_MAKER_TILE (\d+)u", host).group(1))
    assert R.T % R.W == 0 and R.W % R.P == 0 and R.P >= 4
    assert np.gcd(R.UNIT, R.T) == 1 and R.UNIT > R.T


@pytest.mark.parametrize("kind", R.KINDS)
def test_probe_holds_every_structural_byte(kind):
    p, k = R.probe(kind), R.K
    assert 100 <= len(p) <= 200
    words, err = M.read_words(p, k, canonize=False)
    assert err is None
    want = {"fasta": [rb"[ACGT]>[^\n]*>[^\n]*\n", rb">\n>\n", rb"[ACGT]\r\n[ACGT]", rb"[ACGT]\t[ACGT]", rb"N", rb"-", rb"[\x80-\xff]", rb"[acgt]", rb"u", rb"U"],
            "fastq": [rb"\n\+[^\n]*[ACGT]+[^\n]*\n", rb"\n\+[^\n]*\n@[^\n]*>[^\n]*\+", rb"@q\n\n\+\n\n", rb"\n@[^\n]*>[^\n]*@[^\n]*\n", rb"\r\n\+\r\n", rb"[ACGT]\t[ACGT]",
                      rb"N", rb"-", rb"[\x80-\xff]", rb"[acgt]", rb"u", rb"U", rb"\n@\n"]}[kind]
    for pattern in want:
        assert re.search(pattern, b"\n" + p), pattern
    # runs of exactly k - 1, k and k + 1 bases between two resets: 0, 1 and 2 words
    runs = re.search(rb"\n([ACGT]+)N([ACGT]+)-([ACGT]+)[>\n]", p)
    assert [len(g) for g in runs.groups()] == [k - 1, k, k + 1]
    # a control byte leaves no code, so the word goes on: the line with "\r", tab and 0x01 is one run
    line = re.search(rb"GGAT\r\n?TC\tAG\x01CT", p).group(0)
    assert len(M.read_words((b">x\n" if kind == "fasta" else b"@x\n") + line, 10)[0]) == 1
    assert len(words) > 30


@pytest.mark.parametrize("kind,edge,pad", SWEEPS, ids=["%s-%s-%s" % s for s in SWEEPS])
def test_sweep_puts_every_byte_on_both_sides_of_the_edge(kind, edge, pad):
    """and every swept text is well formed, holds the swept bytes where it says, and has the tail's words behind them"""
    e = R.EDGES[edge]
    piece, tail = R.swept(kind, pad), R.tail(kind)
    tail_words = M.read_words(tail, 32)[0]
    assert len(tail) >= R.T + 40 and len(tail_words) > 0 and piece.endswith(R.probe(kind))
    starts = []
    for at, text in R.sweep(kind, e, pad):
        starts.append(at)
        assert text[at:at + len(piece)] == piece and text[at + len(piece):] == tail
        words, err = M.read_words(text, 32)
        assert err is None, at
        assert words[-len(tail_words):] == tail_words, at
    assert 16 < len(starts) <= 260 and starts == list(range(starts[0], e + 2))
    for i in range(len(piece)):
        landed = {at + i for at in starts}
        if edge != "3P" or i <= e - 1 - starts[0]:
            assert e - 1 in landed and e in landed, i
        # (an edge nearer to the start than the piece is long: every byte still meets both sides of a thread's edge that is no wavefront's)
        assert any(p % R.P == R.P - 1 and p % R.W != R.W - 1 for p in landed) and any(p % R.P == 0 and p % R.W for p in landed), i
    # the pad is what it says: a name or a quality line gives no word, a sequence a word per base
    in_front = M.read_words(R.padded(kind, pad, starts[-1], b"", b""), 4)[0]
    assert len(in_front) == {"name": 0, "quality": 3, "sequence": starts[-1] - head_len(kind, pad) - 3}[pad]


def head_len(kind, pad):
    return len(R.padded(kind, pad, len(R._PADS[(kind, pad)][0]), b"", b""))


@pytest.mark.parametrize("variant", R.HOSTILE)
def test_hostile_variants_give_the_error_of_the_table(variant):
    kind, rec, j, byte, want = R.HOSTILE[variant]
    for edge in R.HOSTILE_EDGES:
        e = R.EDGES[edge]
        landed = set()
        for at, text in R.hostile(variant, e):
            landed.add(at)
            assert text[at:at + 1] == byte
            words, err = M.read_words(text, 8)
            if want is None:
                assert err is None and words == M.read_words(text[:at], 8)[0] and M.read_words(text[:at] + rec[j:j + 1] + text[at + 1:], 8) != (words, None)
            else:
                assert err == (want, at)
        assert e - 1 in landed and e in landed


@pytest.mark.parametrize("kind", R.KINDS)
def test_grammar_texts_are_well_formed_and_seldom_wordless(kind):
    wordless, seen = 0, set()
    lengths = set()
    for seed in R.SEEDS:
        text = R.grammar(seed, kind)
        assert text == R.grammar(seed, kind)
        assert R.T <= len(text) <= 3 * R.T and 0 not in text and text[:1] == (b">" if kind == "fasta" else b"@")
        words, err = M.read_words(text, 32)
        assert err is None, seed
        wordless += not words
        subs = IM.read_locations(text, 32)[4] if seed % 10 == 0 else []
        lengths |= {s[3] for s in subs}
        seen |= {name for name, hit in (("crlf", b"\r\n" in text), ("no final newline", text[-1] != 10), ("high byte", max(text) >= 0x80),
                                        ("control byte", bool(re.search(rb"[\x01-\x08\x0b-\x1f]", text))), ("empty name", b"\n" + text[:1] + b"\n" in text or b"\n" + text[:1] + b"\r\n" in text),
                                        ("long name", any(len(l) > R.T and l[:1] == text[:1] for l in text.split(b"\n"))), ("tags in a name", b"a>b@c+d" in text),
                                        ("mid-line >", kind == "fasta" and bool(re.search(rb"[ACGTacgtu]>", text)))) if hit}
    assert wordless * 10 <= len(R.SEEDS), wordless
    assert seen >= {"crlf", "no final newline", "high byte", "control byte", "empty name", "long name", "tags in a name"} | ({"mid-line >"} if kind == "fasta" else set())
    assert len(R.SEEDS) == 200 and set(R.line_lengths(32)) >= {0, 1, R.P - 1, R.P, R.P + 1, 31, 32, 33, 60, R.W - 1, R.W, R.W + 1}
    if kind == "fastq":  # a FastQ sequence is one line: its length is the line's
        assert lengths >= {0, 1, R.P, 32, 60, R.W + 1}


@pytest.mark.parametrize("kind", R.KINDS)
def test_units_expectation_is_the_models_on_the_real_text(kind):
    """five units and a (short) long-named record between them, k = 25: the arrays built by shifting equal what the models
    give for the concatenation"""
    k = 25
    parts = R.units(kind, 5, a=2, name_end=2 * R.UNIT + 3 * R.T + 100)
    assert [r for _, r in parts] == [2, 1, 3]
    text = R.units_text(parts)
    e = R.units_expected(parts, k)
    words, err = M.read_words(text, k)
    assert err is None and len(words) > 5 * 2000
    assert np.array_equal(e["words"], np.array(words, dtype=np.uint64))
    w, o, p, d, s = IM.read_locations(text, k)
    for name, arr in (("words", w), ("ordinals", o), ("positions", p), ("strands", d)):
        assert np.array_equal(e[name], np.array(arr, dtype=np.uint64)), name
    assert np.array_equal(e["subseqs"], np.array(s, dtype=np.uint64))
    assert len(s) > 5 * 5 and len(set(d)) == 2
    assert np.array_equal(R.raw_locations(e), np.array([(a << 33) | (b << 1) | c for a, b, c in zip(o, p, d)], dtype=np.uint64))


@pytest.mark.parametrize("kind", R.KINDS)
def test_units_text_passes_the_scan_s_threads_with_a_name_over_one_thread_s_stretch(kind):
    parts = R.units(kind)
    text = R.units_text(parts)
    assert sum(r for _, r in parts) == R.N_UNITS + 1 and 0 not in text
    tiles = -(-len(text) // R.T)
    per = -(-tiles // R.SCAN)
    assert tiles > R.SCAN and per == 2
    start = parts[0][1] * R.UNIT  # the long name's tag
    end = text.index(b"\n", start)
    name = text[start + 1:end]
    assert b">" not in name and b"ACGT" in name and len(name) >= 3 * R.T
    stretches = [i for i in range(R.SCAN) if start < i * per * R.T and (i + 1) * per * R.T <= end]
    assert stretches, "no thread of the scan has its whole stretch inside the name"
    cuts = R.units_cuts()
    assert start < cuts[0] < end and cuts[0] // R.T == R.SCAN  # in mid-name, in the first tile behind the mark
    assert re.fullmatch(rb"[ACGT]{64}", text[cuts[1] - 32:cuts[1] + 32]) and (cuts[1] + 1) % R.T == 0  # in mid-word
    for piece in (text[:cuts[0]], text):  # the first piece, too, has more tiles than the scan has threads
        assert -(-len(piece) // R.T) > R.SCAN


def stretch_fold(info, forget):
    """k_mk_state_scan's fold of "in a name" restated: a summary per thread's stretch of tiles, a serial pass over the
    summaries, the stretches again from what the pass gives each.  info: per tile ('\\n's, a '>' stands behind the last of
    them); forget: a stretch's summary drops what the tiles in front of a tile without a '\\n' said"""
    per = -(-len(info) // R.SCAN)
    out, name = [], 0
    for i in range(R.SCAN):
        stretch = info[i * per:(i + 1) * per]
        has = tail = 0
        for nl, tl in stretch:
            tail = tl if nl or forget else tail | tl
            has |= nl != 0
        at = name
        for nl, tl in stretch:
            out.append(at)
            at = tl if nl else at | tl
        name = tail if has else name | tail
    return out


def test_units_text_tells_a_fold_that_forgets_inside_a_stretch():
    """the FastA text of more than SCAN tiles gives another "in a name" at some tile when the fold over a thread's stretch
    is wrong in the way a text of one tile per thread cannot show"""
    text = R.units_text(R.units("fasta"))
    info = []
    for t in range(0, len(text), R.T):
        tile = text[t:t + R.T]
        info.append((tile.count(b"\n"), int(b">" in tile[tile.rfind(b"\n") + 1:])))
    truth, name = [], 0
    for nl, tl in info:
        truth.append(name)
        name = tl if nl else name | tl
    assert stretch_fold(info, False) == truth and 0 < sum(truth) < len(truth)
    assert stretch_fold(info, True) != truth
    assert stretch_fold(info[:R.SCAN], True) == truth[:R.SCAN]  # one tile per thread: the same mistake changes nothing
