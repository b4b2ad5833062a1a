#!/usr/bin/env python3
"""What the REFERENCE glistcompare makes of -mm N (difference up to N mismatches).  Needs oracle/_ref/glistcompare;
writes tests/golden/mm_cases.json.

What is committed is DATA ONLY: per case the argv, exit code, stdout and stderr of the reference, and per output file
its sha256 and header totals; per input its recipe (a function of tests/mismatch_util.py and its arguments, or a file
of tests/golden/index_inputs.npz) and sha256.  The two 2 x 2e6-record k = 25 cases take the reference minutes.
Running this again reproduces the JSON byte for byte.

Left out on purpose (documented deviations, covered against tests/mismatch_model.py instead): an empty lookup list
(the reference crashes) and -dd -du (the reference prints an assertion message per lookup)."""
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mismatch_util as MU  # noqa: E402
from genometester4_amd.listio import parse_header, write_list  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "glistcompare")
OUT = os.path.join(HERE, "mm_cases.json")

# name -> recipe: ("dense", seed, k, p_a, p_b) / ("planted", seed, k, n_a) / ("shared_half", seed, n, k) / ("fixture", file)
INPUTS = {
    "d4": ("dense", 11, 4, 0.35, 0.35),
    "d5": ("dense", 12, 5, 0.25, 0.3),
    "p13": ("planted", 13, 13, 1500),
    "p25": ("planted", 25, 25, 1200),
    "p31": ("planted", 31, 31, 800),
    "p32": ("planted", 32, 32, 800),
    "big25": ("shared_half", 2025, 2_000_000, 25),
    "Ia_6": ("fixture", "Ia_6.index"),
    "Ib_6": ("fixture", "Ib_6.index"),
}


def build_inputs(names, where):
    """writes the named inputs into `where`; returns {name: file name}"""
    files = {}
    for name in names:
        r = INPUTS[name]
        if r[0] == "fixture":
            data = np.load(os.path.join(HERE, "index_inputs.npz"))[r[1]].tobytes()
            with open(os.path.join(where, r[1]), "wb") as f:
                f.write(data)
            files[name] = r[1]
            continue
        if r[0] == "dense":
            a, b = MU.dense_pair(r[1], r[2], r[3], r[4])
        elif r[0] == "planted":
            a, b = MU.planted_pair(r[1], r[2], r[3])
        else:
            a, b = MU.shared_half_pair(r[1], r[2], r[3])
        k = r[2] if r[0] != "shared_half" else r[3]
        for side, rec in (("a", a), ("b", b)):
            fn = "%s%s.list" % (name, side)
            write_list(os.path.join(where, fn), rec, k)
            files[name + side] = fn
    return files


def cases():
    """[(id, input name, argv after the two file names)] in a fixed order"""
    out = []
    for inp, k in (("d4", 4), ("d5", 5)):
        for ops in (["-d"], ["-dd"], ["-du"]):
            for n in (1, 2, 3, k + 1):
                for c in ("0", "1", "2", "3", "4294967295"):
                    out.append(("%s%s_mm%d_c%s" % (inp, "".join(ops), n, c), inp, ops + ["-mm", str(n), "-c", c]))
        out.append(("%s_i_d_mm1" % inp, inp, ["-i", "-d", "-mm", "1"]))
        out.append(("%s_u_mm1" % inp, inp, ["-u", "-mm", "1"]))
        out.append(("%s_i_mm2" % inp, inp, ["-i", "-mm", "2", "-o", "nothing"]))
        out.append(("%s_dd_mm2_count" % inp, inp, ["-dd", "-mm", "2", "--count_only"]))
        out.append(("%s_du_mm1_count_c2" % inp, inp, ["-du", "-mm", "1", "-c", "2", "--count_only"]))
        out.append(("%s_dd_mm1_D" % inp, inp, ["-dd", "-mm", "1", "-D", "-o", "dbg"]))
        out.append(("%s_u_mm1_D" % inp, inp, ["-u", "-mm", "1", "-D"]))
    for inp in ("p13", "p25", "p31", "p32"):
        for ops in (["-d"], ["-dd"], ["-du"]):
            for n in (1, 2, 3):
                for c in ("1", "2"):
                    if n == 3 and c == "2":
                        continue
                    out.append(("%s%s_mm%d_c%s" % (inp, "".join(ops), n, c), inp, ops + ["-mm", str(n), "-c", c]))
        out.append(("%s_d_mm1_count" % inp, inp, ["-d", "-mm", "1", "--count_only"]))
    out.append(("idx6_dd_mm1", "Ia_6+Ib_6", ["-dd", "-mm", "1", "-o", "x"]))
    out.append(("idx6_du_mm2_count", "Ia_6+Ib_6", ["-du", "-mm", "2", "--count_only"]))
    out.append(("big25_d_mm1", "big25", ["-d", "-mm", "1"]))
    out.append(("big25_d_mm2", "big25", ["-d", "-mm", "2"]))
    return out


def pair_files(inp, files):
    if "+" in inp:
        x, y = inp.split("+")
        return [files[x], files[y]]
    return [files[inp + "a"], files[inp + "b"]]


def sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def main():
    if not os.path.exists(REF):
        sys.exit("build the reference first: make -C oracle ref")
    work = tempfile.mkdtemp(prefix="gt4mm_")
    try:
        files = build_inputs(list(INPUTS), work)
        golden = {"inputs": {n: {"recipe": list(INPUTS[n][:]), } for n in INPUTS},
                  "input_files_sha256": {fn: sha(os.path.join(work, fn)) for fn in sorted(files.values())},
                  "cases": []}
        for cid, inp, argv in cases():
            run = os.path.join(work, "run")
            os.mkdir(run)
            full = pair_files(inp, files) + argv
            r = subprocess.run([REF] + ["../" + a if a in files.values() else a for a in full], cwd=run, capture_output=True)
            outs = {}
            for name in sorted(os.listdir(run)):
                path = os.path.join(run, name)
                with open(path, "rb") as f:
                    h = parse_header(f.read(48))
                outs[name] = {"sha256": sha(path), "n_words": h["n_words"], "total_count": h["total_count"]}
            shutil.rmtree(run)
            golden["cases"].append({"id": cid, "input": inp, "argv": full, "exit": r.returncode,
                                    "stdout": r.stdout.decode(), "stderr": r.stderr.decode(), "files": outs})
            print(cid, r.returncode, len(outs), flush=True)
        with open(OUT, "w") as f:
            json.dump(golden, f, indent=1, sort_keys=True)
            f.write("\n")
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
