"""The fixtures of tests/golden/gquery_cases.json on disk, and the checks every replay of them shares."""
import base64
import hashlib
import json
import os
import tempfile
import zlib

import numpy as np

import golden_util as G
from genometester4_amd.listio import RECORD_DTYPE, write_list

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINARY = os.path.join(ROOT, "genometester4_amd", "glistquery")
CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "gquery_cases.json")))


def lists():
    """{name: (records, word length)} of every list the cases name"""
    _, inputs, _ = G.load()
    out = {n: (inputs[n][0], inputs[n][1]) for n in CASES["inputs"]}
    for n, (packed, k) in CASES["lists"].items():
        out[n] = (np.frombuffer(zlib.decompress(base64.b64decode(packed)), dtype=RECORD_DTYPE), k)
    return out


def make_workdir():
    d = tempfile.mkdtemp(prefix="gt4gquery_")
    for n, (rec, k) in lists().items():
        write_list(os.path.join(d, n + ".list"), rec, k)
    for n, text in CASES["files"].items():
        with open(os.path.join(d, n), "wb") as f:
            f.write(text.encode("latin-1"))
    return d


def check_stdout(case, stdout: bytes):
    if "stdout" in case:
        assert stdout.decode("latin-1") == case["stdout"], case["id"]
    else:
        assert stdout.decode("latin-1")[:300] == case["stdout_head"], case["id"]
        assert len(stdout) == case["stdout_bytes"], case["id"]
        assert hashlib.sha256(stdout).hexdigest() == case["stdout_sha256"], case["id"]


def parse(argv):
    """the query options of a recorded argv"""
    p = dict(lists=[], mm=0, p=0, min=0, max=0xFFFFFFFF, all=False, q=None, f=None, s=None, l=None, use_3p=False, use_5p=False, other=[])
    i = 0
    while i < len(argv):
        a = argv[i]
        if a in ("-q", "-f", "-s", "-l"):
            if i + 1 >= len(argv) or argv[i + 1].startswith("-"):
                p["other"].append(a)  # the grammar skips the next argument with a warning
            else:
                p[a[1]] = argv[i + 1]
            i += 1
        elif a in ("-mm", "-p", "-min", "-max"):
            try:
                p[a.lstrip("-")] = int(argv[i + 1])
            except (ValueError, IndexError):
                p["other"].append(a)  # one of the grammar's error cases
            i += 1
        elif a in ("--all", "-all"):
            p["all"] = True
        elif a in ("--3p", "--5p"):
            p["use_" + a[2:]] = True
        elif a in ("--bloom", "--disable_scouts"):
            pass
        elif a.startswith("-"):
            p["other"].append(a)
            if a == "--distribution":
                i += 1
        else:
            p["lists"].append(a)
        i += 1
    return p
