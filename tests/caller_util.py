"""The fixtures of tests/golden/caller_cases.json on disk, the seed-built marker tables, and what every replay shares."""
import hashlib
import json
import os
import re
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINARY = os.path.join(ROOT, "genometester4_amd", "gmer_caller")
COUNTER = os.path.join(ROOT, "genometester4_amd", "gmer_counter")
CASES_PATH = os.path.join(ROOT, "tests", "golden", "caller_cases.json")
FULL_STDOUT = 3000  # bytes of a transcript's stdout kept verbatim; above that its SHA-256 and length
ITERATION = re.compile(r"^Iteration (\d+) delta (\S+)$", re.M)


def markers(seed, n_auto, n_x=0, n_y=0, coverage=30.0, male=False, pairs=1, maf=0.3):
    """A table as gmer_counter prints it (ID, N_KMERS, then `pairs` count pairs a line): n_auto autosomal markers "chr:pos",
    n_x of X and n_y of Y.  Counts are Poisson draws around the coverage for the genotype drawn (AA, AB, BB by the allele
    frequency; one copy on a male's X and Y; nothing on a female's Y), around 0.05 for the absent allele; every 97th
    marker has a third copy, every 89th is not covered at all."""
    rng = np.random.default_rng(seed)
    lines = []

    def pair(copies_a, copies_b):
        a = int(rng.poisson(coverage / 2 * copies_a if copies_a else 0.05))
        b = int(rng.poisson(coverage / 2 * copies_b if copies_b else 0.05))
        return a, b

    def one(name, ploidy, i):
        if i % 89 == 88:
            counts = [(0, 0)] * pairs
        else:
            n_b = int(rng.binomial(ploidy, maf))
            n_a = ploidy - n_b + (1 if i % 97 == 96 else 0)
            counts = [pair(n_a, n_b) for _ in range(pairs)]
        lines.append("\t".join([name, str(2 * pairs)] + ["%d\t%d" % c for c in counts]))

    for i in range(n_auto):
        one("%d:%d" % (1 + i % 22, 1000 + 37 * i), 2, i)
    for i in range(n_x):
        one("X:%d" % (5000 + 41 * i), 1 if male else 2, i)
    for i in range(n_y):
        one("Y:%d" % (7000 + 43 * i), 1 if male else 0, i)
    return ("\n".join(lines) + "\n").encode()


def pipeline_db():
    """gmer_util.big_db with its nodes named "1:<n>": --model full takes a line for an autosomal marker by its first byte"""
    import gmer_util
    return gmer_util.big_db().replace(b"\nnode", b"\n1:")


def load_cases():
    return json.load(open(CASES_PATH))


def file_bytes(cases, name):
    spec = cases["files"][name]
    if isinstance(spec, dict):
        if spec["kind"] == "markers":
            return markers(**{k: v for k, v in spec.items() if k != "kind"})
        raise ValueError(spec["kind"])
    return spec.encode("latin-1")


def make_workdir(cases):
    d = tempfile.mkdtemp(prefix="gt4caller_")
    for name in cases["files"]:
        with open(os.path.join(d, name), "wb") as f:
            f.write(file_bytes(cases, name))
    return d


def sha(data):
    return hashlib.sha256(data).hexdigest()


def stdout_matches(case, out: bytes):
    """the case's stdout against `out`: verbatim, or by SHA-256 and length where the generator kept only those"""
    if "stdout" in case:
        return out == case["stdout"].encode("latin-1")
    return len(out) == case["stdout_bytes"] and sha(out) == case["stdout_sha256"]


def iterations(stderr: bytes):
    """the values of the "Iteration N delta V" lines of -D -D, as printed"""
    return [m.group(2) for m in ITERATION.finditer(stderr.decode("latin-1"))]
