"""The fixtures of tests/golden/gqseq_cases.json (made by tests/golden/make_golden_gqseq.py from the reference's glistquery)
on disk, and what the tests of glistquery --per_sequence read out of a recorded argv."""
import base64
import json
import os
import tempfile
import zlib

import numpy as np

from genometester4_amd.listio import RECORD_DTYPE, write_list

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINARY = os.path.join(ROOT, "genometester4_amd", "glistquery")
CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "gqseq_cases.json")))


def lists():
    """{name: (records, word length)}"""
    return {n: (np.frombuffer(zlib.decompress(base64.b64decode(packed)), dtype=RECORD_DTYPE), k) for n, (packed, k) in CASES["lists"].items()}


def make_workdir():
    d = tempfile.mkdtemp(prefix="gt4gqseq_")
    for n, (rec, k) in lists().items():
        write_list(os.path.join(d, n + ".list"), rec, k)
    for n, text in CASES["files"].items():
        with open(os.path.join(d, n), "wb") as f:
            f.write(text.encode("latin-1"))
    return d


def parse(argv):
    """(list name, file name, mm, p, min, max, min_hits) of a computed case's argv"""
    p = {"-mm": 0, "-p": 0, "-min": 0, "-max": 0xFFFFFFFF, "--min_hits": 0, "-s": None}
    lst, i = None, 0
    while i < len(argv):
        if argv[i] in p:
            p[argv[i]] = argv[i + 1] if argv[i] == "-s" else int(argv[i + 1])
            i += 1
        elif not argv[i].startswith("-"):
            lst = argv[i][:-len(".list")]
        else:
            assert argv[i] == "--per_sequence", argv
        i += 1
    return lst, p["-s"], p["-mm"], p["-p"], p["-min"], p["-max"], p["--min_hits"]
