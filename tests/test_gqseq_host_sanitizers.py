"""The host-only helpers glistquery --per_sequence added to csrc/gt4_cli.c (the length of a sequence name in the mapped
file; the byte sizes GT4HIP_QUERY_CHUNK is read with) under AddressSanitizer and UndefinedBehaviorSanitizer, in a
stand-alone program (tests/harness/cli_names_harness.c) linked against the CPU stand-in for the device layer, run as a
process of its own.  No GPU, nothing sanitized is loaded into Python."""
import os
import shutil
import subprocess

import pytest

import seqprofile_model as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genometester4_amd", "csrc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler: the sanitizer run of the command line's helpers cannot be skipped"
    out = str(tmp_path_factory.mktemp("gqseq") / "cli_names_asan")
    src = [os.path.join(ROOT, "tests", "harness", "cli_names_harness.c"), os.path.join(CSRC, "gt4_cli.c"), os.path.join(CSRC, "gt4_listfile.c"),
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


TEXTS = [b">one two\nACGT\n>\nAC\n>tab\there\nACGT\n>last", b"@r\nACGT\n+\nIIII\n@end-of-file-in-the-name", b">\xff\xfe high bytes\nAC\n", b">x", b""]


@pytest.mark.parametrize("text", TEXTS)
def test_name_lengths_at_every_position_and_behind_the_file(harness, tmp_path, text):
    path = str(tmp_path / "names.fa")
    with open(path, "wb") as f:
        f.write(text)
    positions = list(range(len(text) + 3)) + [1 << 40, (1 << 64) - 1]
    want = b"".join(b"%d\t%d\t%s\n" % (p, len(SP.name_of(text, p)) if p < len(text) else 0, SP.name_of(text, p) if p < len(text) else b"") for p in positions)
    assert run(harness, [path] + [str(p) for p in positions]) == want


def test_chunk_sizes(harness):
    got = run(harness, ["--bytes", "1", "7", "64", "2K", "3M", "1G", "", "0", "-5", "x", "12q"]).split()
    assert got[:6] == [b"1", b"7", b"64", b"2048", b"%d" % (3 << 20), b"%d" % (1 << 30)]
    assert got[6:10] == [b"0"] * 4 and got[-1] == b"0"
