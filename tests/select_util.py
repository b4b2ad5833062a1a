"""What the tests of glistcompare -u --min_lists / --max_lists share: the goldens made from the reference binary
(tests/golden/select_cases.json, tests/golden/make_golden_select.py) and the tile sizes of the kernels involved, read from
the sources."""
import base64
import json
import os
import re

import numpy as np

from genometester4_amd.listio import RECORD_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genometester4_amd", "csrc")
RULE_ARGS = {"default": (0, 1), "max": (4, 1), "3": (7, 3)}  # -r STRING -> (rule, count_override)


def _records(b64):
    return np.frombuffer(base64.b64decode(b64), dtype=RECORD_DTYPE).copy()


def load_golden():
    """({name: (word_length, [records per list])}, [case dicts with "expected" records])"""
    with open(os.path.join(ROOT, "tests", "golden", "select_cases.json")) as f:
        g = json.load(f)
    inputs = {n: (v["word_length"], [_records(b) for b in v["lists"]]) for n, v in g["inputs"].items()}
    cases = [dict(c, expected=_records(c["records"])) for c in g["cases"]]
    return inputs, cases


def _define(header, name):
    txt = open(os.path.join(CSRC, header)).read()
    m = re.search(r"#define\s+%s\s+(\d+)" % name, txt)
    assert m, (header, name)
    return int(m.group(1))


def nway_tile():
    """records per tile of the N-way tile kernel (threads x records per thread, gt4hip_nway_tile.h): at most that many rows
    per tile of a ragged count table"""
    return _define("gt4hip_nway_tile.h", "GT4_NWAY_NT") * _define("gt4hip_nway_tile.h", "GT4_NWAY_RPT")


def select_tile():
    """rows the select emit kernel stages at a time (gt4hip_host.h)"""
    return _define("gt4hip_host.h", "GT4HIP_SELECT_TILE")


def select_segment():
    """rows per segment of a contiguous table (gt4hip_host.h)"""
    return _define("gt4hip_host.h", "GT4HIP_SELECT_SEGMENT")
