"""The pair partition's co-rank search (genometester4_amd/csrc/gt4hip_corank.h) on the CPU, without a GPU: the header is
compiled with g++ -fsanitize=address,undefined into tests/harness/corank_model.cc, which runs the two levels of the
partition on key arrays and counts every search's probes, guided and bisected.

Checked on every input of tests/partition_inputs.py and every tile length: both searches give numpy's co-ranks (exactness
does not depend on the keys); no search exceeds the worst case the header states (bisection: ceil (log2 (W + 1)) probes for
a bracket of W records, guided: that and CORANK_GUIDED_MAX, which the program prints with the header's other constants); on
the stride-like and the iid inputs the guided search needs fewer probes than bisection on the mean; and on keys in
stretches no search takes more probes than bisection (the guard at the bracket's ends).  `python tests/test_corank_model.py` prints the mean probe counts."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import partition_inputs as P  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(dirname):
    exe = os.path.join(str(dirname), "corank_model")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "genometester4_amd", "csrc"), os.path.join(ROOT, "tests", "harness", "corank_model.cc"), "-o", exe], check=True)
    return exe


def run_model(exe, dirname, name):
    """{T: (coarse rows, tile rows, constants)}: the columns corank_model.cc prints behind the level letter, as int arrays;
    constants = (PART_COARSE, CORANK_GUIDED_MAX, CORANK_NARROW) as the header has them"""
    ka, kb, _ = P.keys(name)
    fa, fb = os.path.join(str(dirname), name + ".a"), os.path.join(str(dirname), name + ".b")
    ka.astype("<u8").tofile(fa)
    kb.astype("<u8").tofile(fb)
    out = {}
    for T in P.TILES:
        text = subprocess.run([exe, fa, fb, str(T)], capture_output=True, text=True, check=True).stdout.splitlines()
        out[T] = (np.array([[int(x) for x in ln.split()[1:]] for ln in text if ln[0] == "c"], dtype=object),
                  np.array([[int(x) for x in ln.split()[1:]] for ln in text if ln[0] == "t"], dtype=object),
                  tuple(int(x) for x in text[0].split()[1:]))
        assert text[0][0] == "k" and len(out[T][2]) == 3
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("corank_model"))


@pytest.fixture(scope="module")
def model(exe, tmp_path_factory):
    d = tmp_path_factory.mktemp("corank_keys")
    got = {}

    def get(name):
        if name not in got:
            got[name] = run_model(exe, d, name)
        return got[name]
    return get


def bisect_bound(w):
    return int(w).bit_length()  # ceil (log2 (w + 1))


@pytest.mark.parametrize("name", sorted(P.INPUTS))
def test_coranks_and_worst_case(model, name):
    ka, kb, _ = P.keys(name)
    for T in P.TILES:
        coarse, tiles, (part_coarse, guided_max, _) = model(name)[T]
        ref = P.reference(name, T)
        assert len(tiles) == len(ref)
        assert [int(x) for x in tiles[:, 0]] == list(range(len(ref)))
        for cols, what in (((1, 2), "guided"), ((4, 5), "bisected")):
            got = np.array(tiles[:, cols], dtype=np.uint64)
            bad = np.flatnonzero((got != ref).any(axis=1))
            assert not len(bad), (name, T, what, bad[:5], got[bad[:5]], ref[bad[:5]])
        # the coarse boundaries are tile boundaries (before the pull-back: a alone)
        n_c = len(coarse)
        assert n_c == (len(ref) - 1 + part_coarse - 1) // part_coarse + 1
        total = len(ka) + len(kb)
        for c in range(n_c):
            diag = min(c * part_coarse * T, total)
            a = int(np.searchsorted(np.arange(len(ka)) + np.searchsorted(kb, ka, side="left"), diag, side="left"))
            assert int(coarse[c, 1]) == a and int(coarse[c, 3]) == a, (name, T, c)
        # worst case, every search: (probes guided, probes bisected, width)
        for rows, cols in ((coarse, (2, 4, 5)), (tiles, (3, 6, 7))):
            for r in rows:
                pg, pb, w = (int(r[c]) for c in cols)
                assert pb <= bisect_bound(w), (name, T, r)
                assert pg <= bisect_bound(w) + guided_max, (name, T, r)


def mean_probes(rows_tiles, part_coarse):
    """(guided, bisected) mean probes of the tile boundaries that are searched (not the coarse ones themselves)"""
    searched = [r for r in rows_tiles if int(r[0]) % part_coarse]
    if not searched:
        return 0.0, 0.0
    return float(np.mean([int(r[3]) for r in searched])), float(np.mean([int(r[6]) for r in searched]))


@pytest.mark.parametrize("name", P.GUIDABLE)
def test_guided_needs_fewer_probes(model, name):
    for T in P.TILES:
        coarse, tiles, (part_coarse, _, _) = model(name)[T]
        g, b = mean_probes(tiles, part_coarse)
        print("%s T=%d: guided %.2f bisected %.2f probes per tile boundary" % (name, T, g, b))
        assert g < b, (name, T, g, b)
        cg, cb = float(np.mean([int(r[2]) for r in coarse])), float(np.mean([int(r[4]) for r in coarse]))
        print("%s T=%d: guided %.2f bisected %.2f probes per coarse boundary" % (name, T, cg, cb))


def test_stretches_are_bisected_from_the_start(model):
    """keys in stretches between wide gaps: the guard at the bracket's ends (CORANK_STRETCH) keeps the placed probes, which
    the mean slope would waste there, off every search -- no boundary, coarse or fine, takes more probes than bisection"""
    for T in P.TILES:
        coarse, tiles, _ = model("stretches")[T]
        worse = [tuple(r) for r in tiles if int(r[3]) > int(r[6])] + [tuple(r) for r in coarse if int(r[2]) > int(r[4])]
        assert not worse, (T, len(worse), worse[:3])


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        e = build(d)
        print("| input | T | tile boundaries: guided | bisected | coarse boundaries: guided | bisected |")
        print("|---|---|---|---|---|---|")
        for name in sorted(P.INPUTS):
            res = run_model(e, d, name)
            for T in P.TILES:
                coarse, tiles, (part_coarse, _, _) = res[T]
                g, b = mean_probes(tiles, part_coarse)
                cg, cb = float(np.mean([int(r[2]) for r in coarse])), float(np.mean([int(r[4]) for r in coarse]))
                print("| %s | %d | %.2f | %.2f | %.2f | %.2f |" % (name, T, g, b, cg, cb))
