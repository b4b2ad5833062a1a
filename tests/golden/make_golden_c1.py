#!/usr/bin/env python3
"""What the REFERENCE glistcompare makes of BASELINE configs[0] (tests/test_config_c1.py): `--intersection` of two
10^7-entry k=16 lists, `--count_only` and `-o`.  Needs oracle/_ref/glistcompare; writes tests/golden/c1_golden.json.

What is committed is DATA ONLY -- the sha256 of both input files and of the file the reference wrote, its header totals
and its stdout -- because the files are 120 MB each: tests/golden_util.py rebuilds the inputs from their seed."""
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
N, K = 10_000_000, 16


def sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def main():
    if not os.path.exists(REF):
        sys.exit("build the reference first: make -C oracle ref")
    work = tempfile.mkdtemp(prefix="gt4c1_")
    try:
        a, b = GU.c1_lists(N)
        write_list(os.path.join(work, "a.list"), a, K)
        write_list(os.path.join(work, "b.list"), b, K)
        r = subprocess.run([REF, "a.list", "b.list", "--intersection", "--count_only"], cwd=work, capture_output=True)
        assert r.returncode == 0, r.stderr.decode()
        w = subprocess.run([REF, "a.list", "b.list", "--intersection", "-o", "ref"], cwd=work, capture_output=True)
        assert w.returncode == 0, w.stderr.decode()
        out = os.path.join(work, "ref_%d_intrsec.list" % K)
        with open(out, "rb") as f:
            h = parse_header(f.read(48))
        golden = {"entries": N, "word_length": K,
                  "inputs_sha256": {"a.list": sha(os.path.join(work, "a.list")), "b.list": sha(os.path.join(work, "b.list"))},
                  "count_only_stdout": r.stdout.decode(),
                  "intrsec": {"file": os.path.basename(out), "n_words": h["n_words"], "total_count": h["total_count"], "sha256": sha(out)}}
    finally:
        shutil.rmtree(work, ignore_errors=True)
    with open(os.path.join(HERE, "c1_golden.json"), "w") as f:
        json.dump(golden, f, indent=1)
        f.write("\n")
    print("wrote tests/golden/c1_golden.json:", golden["count_only_stdout"].replace("\n", " "))


if __name__ == "__main__":
    main()
