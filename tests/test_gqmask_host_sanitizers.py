"""The hold-back unit of glistquery --mask (GT4MaskTail, csrc/gt4_cli.c) under AddressSanitizer and
UndefinedBehaviorSanitizer, in a stand-alone program (tests/harness/mask_tail_harness.c) linked against the CPU stand-in for
the device layer, run as a process of its own.  The program is fed texts as the library gives them piece by piece (from
tests/mask_model.py: each piece's own covered bases replaced, and its `back`), in pieces of 1, 2, 7 and 64 bytes; what it
writes must be the model's masked text.  No GPU, nothing sanitized is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import mask_model as MM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genometester4_amd", "csrc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler: the sanitizer run of the command line's helpers cannot be skipped"
    out = str(tmp_path_factory.mktemp("gqmask") / "mask_tail_asan")
    src = [os.path.join(ROOT, "tests", "harness", "mask_tail_harness.c"), os.path.join(CSRC, "gt4_cli.c"), os.path.join(CSRC, "gt4_listfile.c"),
           os.path.join(ROOT, "tests", "harness", "gt4hip_stub.c"), os.path.join(ROOT, "oracle", "gt4_oracle.c")]
    r = subprocess.run([cc, "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-I", os.path.join(ROOT, "include")] + src + ["-o", out, "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def run(binary, argv):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=97", UBSAN_OPTIONS="print_stacktrace=1:exitcode=98")
    p = subprocess.run([binary] + argv, capture_output=True, env=env, timeout=60)
    err = p.stderr.decode("latin-1")
    assert "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    assert p.returncode == 0, (p.returncode, err)
    return p.stdout


SEQ = b"ACGTTGCATGCCGATAGCTAGGCTAACGTTAGCCATGGATCGATTACAGGCATCGATCGGATTACCGATGCAGTCAGTCGGATC"
TEXTS = {
    "fasta": b">ACGT name\n" + SEQ[:30] + b"\n" + SEQ[30:61] + b"\n\n" + SEQ[61:] + b"\n>two\nACNNGT" + SEQ[5:50].lower() + b"\r\n",
    "fastq": b"@r ACGT\n" + SEQ[:40] + b"\n+\n" + b"ACGT" * 10 + b"\n@q\n" + SEQ[40:].replace(b"T", b"U") + b"\n+q\n" + b"TGCA" * 11 + b"\n",
    # a run of blank lines and control bytes longer than any piece here, inside a sequence: the words go on behind it
    "blank-run": b">s\n" + SEQ[:35] + b"\n" * 150 + b"\r\t\x01" * 20 + SEQ[35:] + b"\n",
    "nul": b">s\n" + SEQ[:50] + b"\0" + SEQ[50:] + b"\n>t\n" + SEQ + b"\n",
    "no-bases": b">only a name, no end of line",
    "empty": b"",
}
KS = (1, 4, 9, 32)


def hit_list(text, k, every):
    """every `every`-th word of the text"""
    words = MM.read_bases(text, k)[0]
    keys = np.unique(np.array(words[::every] or [0], dtype=np.uint64))
    return keys, np.ones(len(keys), dtype=np.uint32)


@pytest.mark.parametrize("soft", [0, 1], ids=["hard", "soft"])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", list(TEXTS))
def test_what_the_tail_writes_is_the_model_s_masked_text(harness, tmp_path, name, k, soft):
    text = TEXTS[name]
    for every in ((3,) if soft else (1,)):  # every word hits / every third does
        keys, counts = hit_list(text, k, every)
        m = MM.mask_text(keys, counts, text, k, soft=bool(soft))
        assert name in ("no-bases", "empty") or m.counts[1] > 0
        for piece in (1, 2, 7, 64):
            cuts = list(range(piece, len(text), piece))
            backs = m.backs(cuts)
            assert max(backs) <= k - 1 and (k == 1 or name in ("no-bases", "empty") or piece > 7 or max(backs) > 0)
            path = str(tmp_path / "pieces")
            with open(path, "wb") as f:
                f.write(m.own_text(cuts, text, bool(soft)))
            got = run(harness, [path, str(k), str(soft), str(piece)] + [str(b) for b in backs])
            assert got == m.text, (name, k, every, piece)


def test_a_back_that_reaches_in_front_of_the_text_is_an_error(harness, tmp_path):
    path = str(tmp_path / "short")
    with open(path, "wb") as f:
        f.write(b">s\nAC")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:exitcode=97", UBSAN_OPTIONS="exitcode=98")
    p = subprocess.run([harness, path, "9", "0", "2", "0", "0", "5"], capture_output=True, env=env, timeout=60)
    assert p.returncode == 2 and b"Sanitizer" not in p.stderr and b"runtime error" not in p.stderr, p.stderr
