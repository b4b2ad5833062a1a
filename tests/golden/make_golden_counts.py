#!/usr/bin/env python3
"""What the REFERENCE glistcompare makes of counts at the edges of u32 arithmetic: ADD sums of exactly 2^32 and 2^32 + 1,
N-way sums of eight 2^31, cutoffs 0, 1, 2^31 and 2^32 - 1, and `-r <N>` near 2^32.  Needs oracle/_ref/glistcompare;
writes tests/golden/count_edges.json.

What is committed is DATA ONLY: per case the argv, exit code, stdout and stderr of the reference, and per output file
its header totals and sha256; per input file its sha256.  tests/golden_util.count_edge_lists rebuilds the inputs from
their seed (33 lists of about 2e5 records).  Running this again reproduces the JSON byte for byte."""
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import golden_util as GU  # noqa: E402
from genometester4_amd.listio import parse_header, write_list  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "glistcompare")
K = GU.COUNT_EDGE_K

PAIR_OPS = (["-u"], ["-i"], ["-d"], ["-dd"], ["-du"], ["-u", "-i", "-d", "-dd"])
PAIR_RULES = ([], ["-r", "add"], ["-r", "subtract"], ["-r", "min"], ["-r", "max"], ["-r", "first"], ["-r", "second"],
              ["-r", "5"], ["-r", "4294967290"])
PAIR_CUTOFFS = ("0", "1", "2147483648", "4294967295")
NWAY_OPS = (["-u"], ["-i"])
NWAY_LISTS = (3, 8, 33)
NWAY_RULES = ([], ["-r", "add"], ["-r", "max"], ["-r", "min"])
NWAY_CUTOFFS = ("1", "2147483648")


def list_name(j):
    return "L%02d.list" % j


def cases():
    """[(id, argv)] in a fixed order"""
    out = []
    for ops in PAIR_OPS:
        for rule in PAIR_RULES:
            for c in PAIR_CUTOFFS:
                argv = [list_name(0), list_name(1)] + ops + rule + ["-c", c]
                out.append(("pair%s%s_c%s" % ("".join(ops), "_r" + rule[1] if rule else "", c), argv))
    for ops in NWAY_OPS:
        for n in NWAY_LISTS:
            for rule in NWAY_RULES:
                for c in NWAY_CUTOFFS:
                    argv = [list_name(j) for j in range(n)] + ops + rule + ["-c", c]
                    out.append(("nway%d%s%s_c%s" % (n, ops[0], "_r" + rule[1] if rule else "", c), argv))
    return out


def sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def main():
    if not os.path.exists(REF):
        sys.exit("build the reference first: make -C oracle ref")
    work = tempfile.mkdtemp(prefix="gt4edges_")
    try:
        lists = GU.count_edge_lists()
        for j, rec in enumerate(lists):
            write_list(os.path.join(work, list_name(j)), rec, K)
        golden = {"word_length": K, "n_lists": len(lists),
                  "inputs_sha256": {list_name(j): sha(os.path.join(work, list_name(j))) for j in range(len(lists))},
                  "cases": []}
        for cid, argv in cases():
            run = os.path.join(work, "run")
            os.mkdir(run)
            r = subprocess.run([REF] + ["../" + a if a.endswith(".list") else a for a in argv], cwd=run, capture_output=True)
            files = {}
            for name in sorted(os.listdir(run)):
                path = os.path.join(run, name)
                with open(path, "rb") as f:
                    h = parse_header(f.read(48))
                files[name] = {"n_words": h["n_words"], "total_count": h["total_count"], "sha256": sha(path)}
            shutil.rmtree(run)
            golden["cases"].append({"id": cid, "argv": argv, "exit": r.returncode, "stdout": r.stdout.decode(),
                                    "stderr": r.stderr.decode(), "files": files})
    finally:
        shutil.rmtree(work, ignore_errors=True)
    cases_ = golden.pop("cases")
    with open(os.path.join(HERE, "count_edges.json"), "w") as f:  # one case a line
        f.write(json.dumps(golden, indent=1)[:-2] + ',\n "cases": [\n')
        f.write(",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in cases_))
        f.write("\n ]\n}\n")
    golden["cases"] = cases_
    print("wrote tests/golden/count_edges.json: %d cases" % len(golden["cases"]))


if __name__ == "__main__":
    main()
