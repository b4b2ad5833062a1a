#!/usr/bin/env python3
"""What the REFERENCE glistcompare makes of --subset METHOD SIZE --seed N.  Needs oracle/_ref/glistcompare; writes
tests/golden/subset_cases.json.

What is committed is DATA ONLY: per case the argv, exit code, stdout and stderr of the reference and every file it left
(base64: a 48-byte header and at most a few hundred 12-byte records); per input its recipe (the arguments of
tests/subset_model.py's make_list, or a file of tests/golden/index_inputs.npz) and sha256.  Running this again reproduces
the JSON byte for byte.

Only inputs on which the reference terminates: rand_unique with SIZE <= n, rand with SIZE <= sum_counts,
rand_weighted_unique with SIZE <= 0.3 n and counts <= 30 (and a one-record list, whose only ratio is 1).  Every run has
a time limit; one that passes it stops the generator: no case is dropped silently."""
import base64
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
import subset_model as SM  # noqa: E402
from genometester4_amd.listio import write_list  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "glistcompare")
OUT = os.path.join(HERE, "subset_cases.json")
TIMEOUT = 20

# name -> ("list", seed, n, k, max_count) / ("fixture", file of index_inputs.npz)
INPUTS = {
    "u300": ("list", 1, 300, 25, 1),       # counts all 1
    "c300": ("list", 2, 300, 13, 30),
    "big40": ("list", 3, 40, 32, 10000),   # rand: one record spans thousands of items
    "k1": ("list", 4, 3, 1, 5),
    "one": ("list", 5, 1, 25, 7),
    "Ia_6": ("fixture", "Ia_6.index"),
}


def input_records(name):
    """the records of a "list" input"""
    r = INPUTS[name]
    assert r[0] == "list"
    return SM.make_list(*r[1:]), r[3]


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
        else:
            rec, k = input_records(name)
            files[name] = name + ".list"
            write_list(os.path.join(where, files[name]), rec, k)
    return files


def cases():
    """[(id, [input names], argv behind the file names)] in a fixed order"""
    out = []

    def add(cid, inp, argv):
        out.append((cid, inp if isinstance(inp, list) else [inp], argv))

    sums = {n: int(input_records(n)[0]["count"].astype(np.uint64).sum()) for n in INPUTS if INPUTS[n][0] == "list"}
    for inp in ("u300", "c300"):
        n = 300
        for size in (0, 1, n // 3, n - 1, n):
            add("%s_unique_%d" % (inp, size), inp, ["--subset", "rand_unique", str(size), "--seed", "7"])
            add("%s_rand_%d" % (inp, size), inp, ["--subset", "rand", str(size), "--seed", "7"])
        for size in (sums[inp] - 1, sums[inp]):
            add("%s_rand_sum_%d" % (inp, size), inp, ["--subset", "rand", str(size), "--seed", "11"])
        for size in (0, 1, 30, 3 * n // 10):
            add("%s_weighted_%d" % (inp, size), inp, ["--subset", "rand_weighted_unique", str(size), "--seed", "7"])
    for seed in (0, 1, 7, -2, (1 << 32) + 7, (1 << 31) - 1):
        add("u300_unique_100_seed%d" % seed, "u300", ["--subset", "rand_unique", "100", "--seed", str(seed)])
        add("c300_rand_100_seed%d" % seed, "c300", ["--subset", "rand", "100", "--seed", str(seed)])
        add("c300_weighted_60_seed%d" % seed, "c300", ["-ss", "rand_weighted_unique", "60", "--seed", str(seed)])
    for size in (1, 1000, sums["big40"] // 2, sums["big40"]):
        add("big40_rand_%d" % size, "big40", ["--subset", "rand", str(size), "--seed", "3"])
    add("big40_unique_13", "big40", ["--subset", "rand_unique", "13", "--seed", "3"])
    add("big40_weighted_12", "big40", ["--subset", "rand_weighted_unique", "12", "--seed", "5"])
    for m, size in (("rand", 2), ("rand", sums["k1"]), ("rand_unique", 2), ("rand_unique", 3), ("rand_weighted_unique", 0)):
        add("k1_%s_%d" % (m, size), "k1", ["--subset", m, str(size), "--seed", "1"])
    for m, size in (("rand", 1), ("rand", 7), ("rand_unique", 1), ("rand_weighted_unique", 1), ("rand_unique", 0)):
        add("one_%s_%d" % (m, size), "one", ["--subset", m, str(size), "--seed", "9"])
    for m, size in (("rand", 50), ("rand_unique", 50), ("rand_weighted_unique", 20)):
        add("index_%s_%d" % (m, size), "Ia_6", ["--subset", m, str(size), "--seed", "4"])
    add("stream", "c300", ["--subset", "rand", "40", "--seed", "2", "--stream"])
    add("debug", "c300", ["--subset", "rand_unique", "40", "--seed", "2", "-D"])
    add("outdir", "u300", ["--subset", "rand_unique", "40", "--seed", "2", "-o", "dir/name"])
    add("outname_first", "u300", ["-o", "x", "--seed", "2", "--subset", "rand", "40"])
    # the error transcripts
    add("err_two_files", ["u300", "one"], ["--subset", "rand", "10", "--seed", "1"])
    add("err_two_word_lengths", ["u300", "c300"], ["--subset", "rand", "10", "--seed", "1"])
    add("err_unique_above_n", "u300", ["--subset", "rand_unique", "301", "--seed", "1"])
    add("err_weighted_above_n", "u300", ["--subset", "rand_weighted_unique", "301", "--seed", "1"])
    add("err_bad_method", "u300", ["--subset", "random", "10"])
    add("err_size_5x", "u300", ["--subset", "rand", "5x"])
    add("err_no_size", "u300", ["--subset", "rand"])
    add("err_no_method", "u300", ["--subset"])
    add("err_no_seed_value", "u300", ["--subset", "rand", "10", "--seed"])
    return out


def sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def run_case(binary, files, inputs, argv, run, timeout=TIMEOUT, env=None):
    """runs `binary` in the fresh directory `run` (with the sub-directory "dir" of the -o dir/name case); returns
    (exit, stdout, stderr, {relative name: bytes} of every file left)"""
    os.makedirs(os.path.join(run, "dir"))
    full = ["../" + files[i] for i in inputs] + argv
    r = subprocess.run([binary] + full, cwd=run, capture_output=True, timeout=timeout, env=env)
    left = {}
    for base, _, names in os.walk(run):
        for name in names:
            path = os.path.join(base, name)
            with open(path, "rb") as f:
                left[os.path.relpath(path, run)] = f.read()
    shutil.rmtree(run)
    return r.returncode, r.stdout.decode(), r.stderr.decode(), left


def main():
    if not os.path.exists(REF):
        sys.exit("build the reference first: make -C oracle ref")
    work = tempfile.mkdtemp(prefix="gt4ss_")
    try:
        files = build_inputs(list(INPUTS), work)
        golden = {"inputs": {n: {"recipe": list(INPUTS[n]), "file": files[n], "sha256": sha(os.path.join(work, files[n]))} for n in INPUTS},
                  "cases": []}
        for cid, inputs, argv in cases():
            try:
                code, out, err, left = run_case(REF, files, inputs, argv, os.path.join(work, "run"))
            except subprocess.TimeoutExpired:
                sys.exit("case %s: the reference ran into its time limit of %d s: choose an input on which it terminates" % (cid, TIMEOUT))
            golden["cases"].append({"id": cid, "inputs": inputs, "argv": argv, "exit": code, "stdout": out, "stderr": err,
                                    "files": {n: base64.b64encode(b).decode() for n, b in sorted(left.items())}})
            print(cid, code, sorted(left), flush=True)
        with open(OUT, "w") as f:
            json.dump(golden, f, indent=1, sort_keys=True)
            f.write("\n")
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
