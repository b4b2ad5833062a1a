"""The fixtures of tests/golden/gindex_cases.json: the texts (kept verbatim or rebuilt from a seed) and the reference's
index files (tests/golden/gindex_files.npz, or a SHA-256 of the masked bytes where a file is large)."""
import json
import os

import numpy as np

import gmaker_util as U

ROOT = U.ROOT
CASES_PATH = os.path.join(ROOT, "tests", "golden", "gindex_cases.json")
FILES_PATH = os.path.join(ROOT, "tests", "golden", "gindex_files.npz")


def random_bases(seed, n):
    return "".join(np.array(list("ACGT"), dtype="U1")[np.random.default_rng(seed).integers(0, 4, size=n)].tolist())


def file_bytes(cases, name):
    spec = cases["files"][name]
    if isinstance(spec, dict):
        if spec["kind"] == "big":
            return U.big_fasta(spec["seed"], spec["n_bases"])
        if spec["kind"] == "one":  # one sequence of n_bases in lines of 70
            t = random_bases(spec["seed"], spec["n_bases"])
            return (">one long sequence\n" + "".join(t[j:j + 70] + "\n" for j in range(0, len(t), 70))).encode()
        if spec["kind"] == "many":  # n one-line sequences of 8 bases: 300 of them lie inside one 4096-byte tile
            t = random_bases(spec["seed"], 8 * spec["n"])
            return "".join(">%d\n%s\n" % (j, t[8 * j:8 * j + 8]) for j in range(spec["n"])).encode()
        if spec["kind"] == "long_name":
            return (">" + "name " * (spec["name_bytes"] // 5) + "\n" + random_bases(spec["seed"], 200) + "\n>after\n" + random_bases(spec["seed"] + 1, 90) + "\n").encode()
        raise ValueError(spec)
    return spec.encode("latin-1")


def load():
    cases = json.load(open(CASES_PATH))
    files = np.load(FILES_PATH)
    return cases, {k: files[k].tobytes() for k in files.files}
