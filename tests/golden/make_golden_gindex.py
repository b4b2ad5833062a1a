#!/usr/bin/env python3
"""Golden index files of the reference's glistmaker --index (reference src/glistmaker.c:366-782) for tests/index_model.py
and the GPU tests.  Needs oracle/_ref/glistmaker (make -C oracle ref).  Writes data only:

    tests/golden/gindex_cases.json   files {name: text (latin-1) | {kind, seed, ...}: tests/gindex_util.file_bytes}
                                     cases [{id, argv, inputs, k, lo, hi, exit, output, bytes, sha256 of the masked file}]
    tests/golden/gindex_files.npz    {case id: the masked bytes} of every index of at most KEEP bytes

Every file is stored with the four undefined bytes of its file block zeroed (tests/index_model.MASKED)."""
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
import gindex_util as G  # noqa: E402
import index_model as IM  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "glistmaker")
KEEP = 40_000


def texts():
    f = {}
    f["multi.fa"] = (">one first sequence\nACGTTGCAAGGCTTAACCGGTTAAGGCCTTAGCTAGCTAGGATCCGATCGATTACGCGCGATATCG\nGGATCCTTAAGGCCAATTGGCCAATTCCGG\nacgtuuacgguacgtUUACG\n"
                     ">two\nACGTNNNNNNACGTACGTACGTTTGACCANACGTAGCTAGCTAGGCTAGCTAGGATCGATCGGCTAGCTAGCTA\n>short\nACG\n>empty\n>three mid>line\nACGTACGGTAC>GTA in a name ACGT\n"
                     "TTGACCAGGTACCAGTTGACCAGGTACCAGTTGACCAGGTAC\n")
    f["crlf.fa"] = ">crlf one\r\nACGTTGCAAGGCTTAACCGGTTAAGGCC\r\nTTAGCTAGCTAGGATCCGATCGATTACGCGCGATATCG\r\n>crlf two\r\nGGATCCTTAAGGCCAATTGGCC\tAATTCCGG\r\n"
    f["nofinal.fa"] = ">no final newline\nACGTTGCAAGGCTTAACCGGTTAAGGCCTTAGCTAGCTAGGATCCGATCG\nATTACGCGCGATATCGGGATCCTTAAGG"
    f["reads.fq"] = ("@r1 first\nACGTTGCAAGGCTTAACCGGTTAAGGCCTTAGCTAGCTAGG\n+\n@IIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n"
                     "@r2\nGGATCCTTAAGGCCAATTGGNCAATTCCGGACGTACGTAA\n+r2 again\n>III+IIIIIIIIIIII@IIIIIIIIIIIIIIIIIIIIII\n"
                     "@r3 with > in sequence\nACGTTGCAAGGCTTAACC>GGTTAAGGCCTTAGCTAGCTAGGATCCGATCGATTACGCGCGATATCG\n+\n+III@III>IIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n")
    f["second.fa"] = ">second file\nTTAGCTAGCTAGGATCCGATCGATTACGCGCGATATCGACGTTGCAAGGCTTAACCGGTTAAGGCC\nACGTACGTACGTACGTACGTACGTACGTACGTACGTAC\n"
    f["lowc.fa"] = ">poly\n" + "A" * 300 + "\n>tandem\n" + "ACGT" * 90 + "\n>palindromes\nACGTACGTTGCATGCAAATTAATT\n" + ">tandem again\n" + "ACGT" * 40 + "\n"
    f["many.fa"] = dict(kind="many", seed=11, n=300)
    f["pos255.fa"] = dict(kind="one", seed=12, n_bases=266)     # k = 11: the largest position is 255, eight bits
    f["pos256.fa"] = dict(kind="one", seed=12, n_bases=267)     # ... 256, nine bits
    f["long.fa"] = dict(kind="one", seed=13, n_bases=20_000)
    f["long_name.fa"] = dict(kind="long_name", seed=14, name_bytes=5000)
    f["big.fa"] = dict(kind="big", seed=4242, n_bases=130_000)
    return f


def main():
    if not os.path.exists(REF):
        sys.exit("build the reference first: make -C oracle ref")
    doc = dict(files=texts(), cases=[])
    work = tempfile.mkdtemp(prefix="gt4gindex_")
    for name in doc["files"]:
        with open(os.path.join(work, name), "wb") as fh:
            fh.write(G.file_bytes(doc, name))
    kept = {}

    def run(cid, inputs, k, extra=(), lo=1, hi=0xffffffff):
        argv = list(inputs) + ["-w", str(k), "-o", cid, "--index"] + list(extra)
        p = subprocess.run([REF] + argv, cwd=work, capture_output=True, timeout=300)
        assert p.returncode == 0, (cid, p.returncode, p.stderr)
        out = "%s_%d.index" % (cid, k)
        data = IM.masked(open(os.path.join(work, out), "rb").read())
        doc["cases"].append(dict(id=cid, argv=argv, inputs=list(inputs), k=k, lo=lo, hi=hi, exit=0, output=out, bytes=len(data), sha256=hashlib.sha256(data).hexdigest()))
        if len(data) <= KEEP:
            kept[cid] = np.frombuffer(data, dtype=np.uint8)

    for k in (1, 2, 11, 16, 31, 32):
        for name in ("multi.fa", "reads.fq"):
            run("%s_k%d" % (name.split(".")[0], k), [name], k)
    run("many_k5", ["many.fa"], 5)
    run("many_k11", ["many.fa"], 11)  # no sequence holds a word: a header alone (write_index_header, :576-626)
    for name in ("crlf.fa", "nofinal.fa", "pos255.fa", "pos256.fa", "long_name.fa"):
        run("%s_k11" % name.split(".")[0], [name], 11)
    run("two_files_k16", ["multi.fa", "reads.fq"], 16)
    run("three_files_k11", ["multi.fa", "reads.fq", "second.fa"], 11)
    for k in (2, 11):
        run("lowc_k%d" % k, ["lowc.fa"], k)
    run("lowc_c2_k11", ["lowc.fa"], 11, ["-c", "2"], lo=2)
    run("lowc_max3_k11", ["lowc.fa"], 11, ["--max", "3"], hi=3)
    run("lowc_c2_max3_k11", ["lowc.fa"], 11, ["-c", "2", "--max", "3"], lo=2, hi=3)
    run("multi_c2_k2", ["multi.fa", "second.fa"], 2, ["-c", "2"], lo=2)
    run("long_k16", ["long.fa"], 16)
    run("big_k25", ["big.fa"], 25)
    shutil.rmtree(work, ignore_errors=True)
    with open(G.CASES_PATH, "w") as fh:
        json.dump(doc, fh, indent=0, sort_keys=True)
    np.savez_compressed(G.FILES_PATH, **kept)
    print("%d cases (%d kept whole), %d + %d bytes" % (len(doc["cases"]), len(kept), os.path.getsize(G.CASES_PATH), os.path.getsize(G.FILES_PATH)))


if __name__ == "__main__":
    main()
