"""The fixtures of tests/golden/gmaker_cases.json on disk, the seed-built large text, and what every replay shares."""
import hashlib
import json
import os
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINARY = os.path.join(ROOT, "genometester4_amd", "glistmaker")
CASES_PATH = os.path.join(ROOT, "tests", "golden", "gmaker_cases.json")


def big_fasta(seed=4242, n_bases=130_000):
    """a FastA text above 100,000 bytes (the reference runs its threads there): three sequences, lines of 61 bases, some N"""
    rng = np.random.default_rng(seed)
    out = []
    for s, n in enumerate((n_bases // 2, n_bases // 3, n_bases - n_bases // 2 - n_bases // 3)):
        codes = rng.integers(0, 4, size=n)
        seq = np.array(list("ACGT"), dtype="U1")[codes]
        seq[rng.integers(0, n, size=n // 5000)] = "N"
        txt = "".join(seq.tolist())
        out.append(">seq%d generated from seed %d\n" % (s, seed))
        out += [txt[j:j + 61] + "\n" for j in range(0, n, 61)]
    return "".join(out).encode()


def load_cases():
    return json.load(open(CASES_PATH))


def file_bytes(cases, name):
    spec = cases["files"][name]
    if isinstance(spec, dict):
        return big_fasta(spec["seed"], spec["n_bases"])
    return spec.encode("latin-1")


def make_workdir(cases):
    d = tempfile.mkdtemp(prefix="gt4gmaker_")
    os.mkdir(os.path.join(d, "dir"))
    for name in cases["files"]:
        with open(os.path.join(d, name), "wb") as f:
            f.write(file_bytes(cases, name))
    return d


def sha(data):
    return hashlib.sha256(data).hexdigest()
