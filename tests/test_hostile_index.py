"""GT4I files whose header or file block points outside the file: gt4_indexfile_open must answer GT4_LISTFILE_ESIZE with
a message and read nothing out of bounds.  The reader (csrc/gt4_listfile.c) and a stand-alone program that calls it and
its walkers (tests/harness/index_reader_harness.c) are compiled with AddressSanitizer and UndefinedBehaviorSanitizer and
run as a process of their own; the same files through the command line, with no device, are exit 1.  No GPU."""
import os
import shutil
import struct
import subprocess

import pytest

import gqloc_util as U

ROOT = U.ROOT
ESIZE = 4
GOOD = U.GFILES["two_files_k16"]  # two files, FastA and FastQ, k = 16
HDR = struct.Struct("<4I2Q4I3Q")


def patched(**kw):
    """GOOD with header fields replaced"""
    names = ("code", "major", "minor", "k", "num_words", "num_locations", "file_bits", "subseq_bits", "pos_bits", "filler", "files_start", "kmers_start",
             "locations_start")
    h = dict(zip(names, HDR.unpack_from(GOOD, 0)))
    h.update(kw)
    return HDR.pack(*[h[n] for n in names]) + GOOD[HDR.size:]


def block_patched(offset, fmt, value, cut=None):
    """GOOD with a field of its file block replaced (offset from files_start), optionally cut behind `cut` bytes of the block"""
    at = HDR.unpack_from(GOOD, 0)[10]
    b = bytearray(GOOD)
    struct.pack_into(fmt, b, at + offset, value)
    return bytes(b if cut is None else b[:at + cut])


def hostile():
    size = len(GOOD)
    f_at = HDR.unpack_from(GOOD, 0)[10]
    name_len = struct.unpack_from("<H", GOOD, f_at + 32)[0]
    return {
        "locations_past_the_end": patched(locations_start=size + 8),
        "locations_start_huge": patched(locations_start=(1 << 64) - 8),
        "num_locations_2_61_plus_1": patched(num_locations=(1 << 61) + 1),     # x 8 wraps to 8
        "num_locations_one_too_many": patched(num_locations=HDR.unpack_from(GOOD, 0)[5] + 1),
        "files_start_past_the_end": patched(files_start=size + 1),
        "files_start_huge": patched(files_start=(1 << 64) - 4),
        "name_length_leads_out": block_patched(32, "<H", 0xFFFF, cut=16 + 18 + 40),
        "name_without_nul": block_patched(32 + 2 + name_len - 1, "<B", 0x41),
        "n_seqs_leads_out": block_patched(24, "<Q", size),                       # x 28 is far more than the file
        "n_seqs_wraps": block_patched(24, "<Q", (1 << 64) // 28 + 1),
        "n_files_too_many": block_patched(12, "<I", 1000),
        "bit_widths_sum_65": patched(file_bits=1, subseq_bits=31, pos_bits=32),
        "bit_width_wraps": patched(file_bits=0xFFFFFFFF, subseq_bits=1, pos_bits=1),
        "block_truncated_in_head": GOOD[:f_at + 10],
        "block_truncated_in_file_entry": GOOD[:f_at + 16 + 9],
        "block_truncated_in_sequences": block_patched(0, "<I", struct.unpack_from("<I", GOOD, f_at)[0], cut=16 + 18 + name_len + 30),
    }


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler: the sanitizer run of the index reader cannot be skipped"
    out = str(tmp_path_factory.mktemp("hostile") / "index_reader_asan")
    r = subprocess.run([cc, "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "harness", "index_reader_harness.c"), os.path.join(ROOT, "genometester4_amd", "csrc", "gt4_listfile.c"), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def _harness(binary, path):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=97", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    p = subprocess.run([binary, path], capture_output=True, env=env, timeout=60)
    err = p.stderr.decode("latin-1")
    assert "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    return p.returncode, p.stdout.decode(), err


def test_the_good_file_opens_and_walks(harness, tmp_path):
    path = str(tmp_path / "good.index")
    open(path, "wb").write(GOOD)
    rc, out, err = _harness(harness, path)
    assert rc == 0 and out.startswith("rc=0\nok files=2 sequences=9 "), (out, err)
    for cid in ("many_k11", "long_name_k11", "three_files_k11", "multi_k1"):  # an index without a file block among them
        open(path, "wb").write(U.GFILES[cid])
        rc, out, err = _harness(harness, path)
        assert rc == 0 and out.startswith("rc=0\nok files="), (cid, out, err)


@pytest.mark.parametrize("name", sorted(hostile()))
def test_hostile_index_is_refused_in_bounds(name, harness, tmp_path):
    path = str(tmp_path / (name + ".index"))
    open(path, "wb").write(hostile()[name])
    rc, out, err = _harness(harness, path)
    assert rc == 0 and out == "rc=%d\n" % ESIZE, (out, err)
    assert err.startswith("gt4_index_map_new: ") and path not in out, err
    # the command line, no device: every form that reads the index
    for argv in ([path, "--files"], [path, "--sequences"], [path, "--locations"], [path], [path, "--stat"], [path, "-q", "A" * 16, "--locations"]):
        p = U.run(argv, str(tmp_path), hide_gpu=True)
        assert p.returncode == 1 and p.stdout == b"" and b"invalid or corrupted" in p.stderr, (argv, p.stderr)


def test_dump_stops_at_a_first_location_outside_the_section(tmp_path):
    """the sections fit the file but the k-mer table points past the locations: the host dump may not follow it"""
    k_at = HDR.unpack_from(GOOD, 0)[11]
    b = bytearray(GOOD)
    struct.pack_into("<Q", b, k_at + 16 * 3 + 8, 1 << 40)
    path = str(tmp_path / "wild.index")
    open(path, "wb").write(bytes(b))
    p = U.run([path, "--locations"], str(tmp_path), hide_gpu=True)
    assert p.returncode == 1 and b"corrupted" in p.stderr
