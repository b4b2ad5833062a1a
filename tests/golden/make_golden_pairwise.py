#!/usr/bin/env python3
"""What `glistcompare L1 .. LN --pairwise` has to print, from outputs of the REFERENCE glistcompare alone.  Needs
oracle/_ref/glistcompare; writes tests/golden/pairwise_cases.json.

The reference has no such option, but every number of it is a line of `--count_only` runs of pairs of lists:
  Li Lj -i --count_only    NUnique = shared[i][j], NTotal = min_total[i][j] (the default rule of the intersection keeps the
                           smaller count); with j = i: the diagonal, a list's words and the sum of its counts
  Li Lj -u --count_only    NUnique = the size of the union (its NTotal carries a 32-bit wraparound per record: recorded, not
                           compared)
  Li Lj -d --count_only    NUnique = the words of Li alone; and Lj Li -d for those of Lj
for every i < j, and Li Li -i for every i.  Every stored count is at least 1: a record with count 0 would be a word of the
reference's intersection (tests/pairwise_model.py says what it means here).

What is committed is DATA ONLY: the input lists (base64 of the 12-byte records) and the numbers the reference printed.
Running this again reproduces the JSON byte for byte."""
import base64
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from genometester4_amd.listio import RECORD_DTYPE, make_records, write_list  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "glistcompare")
OUT = os.path.join(HERE, "pairwise_cases.json")
TOP = 0xffffffff


def random_lists(n, k, universe, seed, max_count=5):
    """n lists over one universe of words: list j holds a word with a probability of its own"""
    rng = np.random.default_rng(seed)
    space = 1 << (2 * k)
    words = np.unique(rng.integers(0, space, size=universe, dtype=np.uint64))
    if k == 32:
        words[-1] = np.uint64(space - 1)  # the all-ones word
    depth = rng.random(len(words))
    lists = []
    for j in range(n):
        m = rng.random(len(words)) < 0.15 + depth
        lists.append(make_records(words[m], rng.integers(1, max_count + 1, size=int(m.sum()), dtype=np.uint32)))
    return lists


def cases():
    """{name: (word_length, lists)}"""
    out = {}
    out["k1_n3"] = (1, [make_records([0, 1, 3], [2, 7, 1]), make_records([1, 2, 3], [3, 1, 9]), make_records([0, 1, 2, 3], [1, 1, 1, 1])])
    out["k16_n6"] = (16, random_lists(6, 16, 120, 16))
    out["k25_n2"] = (25, random_lists(2, 25, 90, 25))
    out["k32_n4"] = (32, random_lists(4, 32, 100, 32))
    base = random_lists(1, 25, 80, 99)[0]
    other = random_lists(1, 25, 80, 98)[0]
    other = other[~np.isin(other["key"], base["key"])]
    # an empty list, two identical lists (0, 1), two disjoint lists (0, 3), and one that overlaps both
    out["k25_n5_shapes"] = (25, [base, base.copy(), np.zeros(0, dtype=RECORD_DTYPE), other, np.sort(np.concatenate([base[::3], other[::2]]), order="key")])
    # counts near 2^32 - 1: the smaller of two counts never wraps, the sums pass 2^32 within three rows.  No two counts of a word
    # add up to 2^32: the reference's union drops a record whose 32-bit sum wraps to 0, below its cutoff of 1
    keys = np.arange(10, 90, 10, dtype=np.uint64)
    out["k16_n3_top"] = (16, [make_records(keys, [TOP, TOP, TOP, TOP - 1, 5, TOP, 2, TOP]),
                              make_records(keys[:6], [TOP, TOP - 2, TOP, TOP, TOP, 7]),
                              make_records(keys[1:], [TOP, TOP, 3, TOP - 1, TOP, TOP, TOP])])
    return out


def run(argv, cwd):
    r = subprocess.run([REF] + argv + ["--count_only"], cwd=cwd, capture_output=True, timeout=60)
    m = re.fullmatch(r"NUnique\t(\d+)\nNTotal\t(\d+)\n", r.stdout.decode())
    if r.returncode or not m:
        sys.exit("reference failed: %s\n%s%s" % (" ".join(argv), r.stdout.decode(), r.stderr.decode()))
    return [int(m.group(1)), int(m.group(2))]


def main():
    if not os.path.exists(REF):
        sys.exit("build the reference first: make -C oracle ref")
    work = tempfile.mkdtemp(prefix="gt4pw_")
    golden = {"cases": []}
    try:
        for name, (k, lists) in cases().items():
            assert 2 <= len(lists) <= 6 and all(len(l) == 0 or int(l["count"].min()) >= 1 for l in lists)
            d = os.path.join(work, name)
            os.makedirs(d)
            files = ["L%d.list" % j for j in range(len(lists))]
            for f, rec in zip(files, lists):
                write_list(os.path.join(d, f), rec, k)
            case = {"id": name, "word_length": k, "lists": [base64.b64encode(l.tobytes()).decode() for l in lists], "diagonal": [], "pairs": []}
            for i in range(len(lists)):
                case["diagonal"].append({"i": i, "intersection": run([files[i], files[i], "-i"], d)})
                for j in range(i + 1, len(lists)):
                    case["pairs"].append({"i": i, "j": j, "intersection": run([files[i], files[j], "-i"], d), "union": run([files[i], files[j], "-u"], d),
                                          "difference_ij": run([files[i], files[j], "-d"], d), "difference_ji": run([files[j], files[i], "-d"], d)})
            golden["cases"].append(case)
            print(name, len(lists), [p["intersection"] for p in case["pairs"]], flush=True)
        with open(OUT, "w") as f:
            json.dump(golden, f, indent=1, sort_keys=True)
            f.write("\n")
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
