"""genometester4_amd/glistquery on a GT4I index WITHOUT a device: --files, --sequences and the dump with --locations are
file I/O on the mapping and must print the reference's bytes (tests/golden/gqloc_cases.json) with the GPU hidden; so
must the errors the reference raises before it looks anything up."""
import os
import shutil

import pytest

import gqloc_util as U
import locations_model as L

NO_DEVICE = [c for c in U.CASES["cases"] if c["id"].startswith(("files_", "sequences_", "dump_", "l_index_"))]


@pytest.fixture(scope="module")
def workdir():
    d = U.make_workdir()
    yield d
    shutil.rmtree(d, ignore_errors=True)


@pytest.mark.parametrize("case", NO_DEVICE, ids=lambda c: c["id"])
def test_no_device_cases_replay(case, workdir):
    assert len(NO_DEVICE) >= 35
    p = U.run(case["argv"], workdir, hide_gpu=True)
    assert p.returncode == case["exit"], p.stderr.decode("latin-1")
    U.check_stdout(case, p.stdout)
    if "stderr" in case:  # the reference's line first; a second line names the option
        assert p.stderr.decode("latin-1").startswith(case["stderr"])
        assert ("--files" if "--files" in case["argv"] else "--sequences") in p.stderr.decode("latin-1")


def test_locations_on_a_list_is_refused_without_a_device(workdir):
    """a deliberate difference: the reference ignores --locations on a .list"""
    for argv in (["Q11.list", "--locations"], ["Q11.list", "--locations", "-q", "ACGTTGCAAGG"], ["Q11.list", "-l", "Q11.list", "--locations", "-mm", "1"],
                 [U.BY_ID["multi_k11"]["output"], "Q11.list", "--locations"]):
        p = U.run(argv, workdir, hide_gpu=True)
        assert p.returncode == 1 and p.stdout == b"", argv
        assert b"--locations" in p.stderr and b"Q11.list is a list" in p.stderr and b"GPU" not in p.stderr, p.stderr


def test_a_query_with_locations_needs_a_device(workdir):
    p = U.run([U.BY_ID["multi_k11"]["output"], "-q", "ACGTTGCAAGG", "--locations"], workdir, hide_gpu=True)
    assert p.returncode == 1 and p.stdout == b"" and b"GPU" in p.stderr  # no CPU path


def test_a_missing_source_gives_the_message_and_empty_names(workdir, tmp_path):
    name = U.BY_ID["two_files_k16"]["output"]
    shutil.copy(os.path.join(workdir, name), tmp_path / name)
    shutil.copy(os.path.join(workdir, "reads.fq"), tmp_path / "reads.fq")  # multi.fa is not there
    p = U.run([name, "--sequences"], str(tmp_path), hide_gpu=True)
    want, missing = L.print_sequences(L.Index(U.GFILES["two_files_k16"]), str(tmp_path))
    assert p.returncode == 0 and p.stdout.decode("latin-1") == want
    assert missing and set(missing) == {"multi.fa"}
    assert p.stderr.decode().count("imap_map_src: could not mmap file multi.fa\n") == len(missing)
    lines = p.stdout.decode().split("\n")
    assert lines[0].split("\t")[:3] == ["0", "0", ""] and "r1 first" in p.stdout.decode()
    q = U.run([name, "--files"], str(tmp_path), hide_gpu=True)  # --files reads no source
    assert q.returncode == 0 and q.stdout.decode() == L.print_files(L.Index(U.GFILES["two_files_k16"])) and q.stderr == b""


def test_an_index_without_locations_option_is_the_list_it_holds(workdir):
    """no query, no --locations: the dump of one list, as before"""
    name = U.BY_ID["lowc_k11"]["output"]
    p = U.run([name], workdir, hide_gpu=True)
    assert p.returncode == 0 and p.stdout.decode() == L.dump(L.Index(U.GFILES["lowc_k11"]), False)
    assert "AAAAAAAAAAA\t290\n" in p.stdout.decode()
