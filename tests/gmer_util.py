"""The fixtures of tests/golden/gmer_cases.json on disk, the seed-built reads and database, and what every replay shares."""
import hashlib
import json
import os
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINARY = os.path.join(ROOT, "genometester4_amd", "gmer_counter")
CASES_PATH = os.path.join(ROOT, "tests", "golden", "gmer_cases.json")
FULL_STDOUT = 3000  # bytes of a transcript's stdout kept verbatim; above that its SHA-256 and length

BASES = np.array(list("ACGT"), dtype="U1")
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def revcomp_text(s):
    return "".join(COMP[c] for c in reversed(s))


def big_reads(seed=77, n_reads=900, read_len=101):
    """FastQ above 100,000 bytes: reads cut out of one random genome of 6,000 bases (so that k-mers recur), an N in every
    23rd read, N in some names and quality lines (gmer_counter --stats counts those as well)"""
    rng = np.random.default_rng(seed)
    genome = "".join(BASES[rng.integers(0, 4, size=6000)].tolist())
    out = []
    for r in range(n_reads):
        at = int(rng.integers(0, len(genome) - read_len))
        seq = genome[at:at + read_len]
        if r % 23 == 0:
            p = int(rng.integers(0, read_len))
            seq = seq[:p] + "N" + seq[p + 1:]
        if r % 2:
            seq = revcomp_text(seq.replace("N", "A"))
        qual = "I" * read_len if r % 7 else "N" + "I" * (read_len - 1)
        out.append("@read%d %s\n%s\n+\n%s\n" % (r, "N" if r % 5 == 0 else "x", seq, qual))
    return "".join(out).encode()


def big_db(seed=78, n_nodes=1200, k=25, reads_seed=77):
    """a text database of n_nodes nodes with 2 to 4 k-mers each (a few thousand k-mers): most cut out of big_reads's genome,
    every fifth node random (absent from the reads); no canonical word twice"""
    rng = np.random.default_rng(reads_seed)
    genome = "".join(BASES[rng.integers(0, 4, size=6000)].tolist())
    rng = np.random.default_rng(seed)
    seen, lines = set(), ["# generated: seed %d, %d nodes, k = %d" % (seed, n_nodes, k)]
    for node in range(n_nodes):
        kmers = []
        while len(kmers) < 2 + node % 3:
            if node % 5 == 4:
                s = "".join(BASES[rng.integers(0, 4, size=k)].tolist())
            else:
                at = int(rng.integers(0, len(genome) - k))
                s = genome[at:at + k]
            canon = min(s, revcomp_text(s))
            if canon in seen:
                continue
            seen.add(canon)
            kmers.append(s if node % 2 else revcomp_text(s))
        lines.append("\t".join(["node%d" % node, str(len(kmers))] + kmers))
    return ("\n".join(lines) + "\n").encode()


def load_cases():
    return json.load(open(CASES_PATH))


def file_bytes(cases, name):
    spec = cases["files"][name]
    if isinstance(spec, dict):
        kind = spec["kind"]
        if kind == "reads":
            return big_reads(spec["seed"], spec["n_reads"], spec["read_len"])
        if kind == "db":
            return big_db(spec["seed"], spec["n_nodes"], spec["k"], spec["reads_seed"])
        if kind == "repeat":  # a name line, then one base n times
            return (">%s\n" % spec["name"]).encode() + spec["base"].encode() * spec["n"] + b"\n"
        raise ValueError(kind)
    return spec.encode("latin-1")


def make_workdir(cases):
    d = tempfile.mkdtemp(prefix="gt4gmer_")
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
