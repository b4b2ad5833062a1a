"""The fixtures of tests/golden/gqloc_cases.json on disk: the reference-built indexes of gindex_files.npz under their
output names, the source texts beside them, the query files and the query list; and the indexes a replay builds itself."""
import json
import os
import subprocess
import tempfile

import numpy as np

import gindex_util as G
import gmaker_util
import gquery_util as U
from genometester4_amd.listio import make_records, write_list

ROOT = U.ROOT
BINARY = U.BINARY
CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "gqloc_cases.json")))
LIST_K = 11
GCASES, GFILES = G.load()
BY_ID = {c["id"]: c for c in GCASES["cases"]}
check_stdout = U.check_stdout


def needs_built(case):
    return any(a == BY_ID[b]["output"] for a in case["argv"] for b in CASES["built"])


def make_workdir(built=None):
    """built: None (the cases on long_k16 / big_k25 cannot run), "model" (tests/index_model.py writes the two files) or
    "cli" (genometester4_amd/glistmaker --index does, on the GPU)"""
    d = tempfile.mkdtemp(prefix="gt4gqloc_")
    for name in GCASES["files"]:
        with open(os.path.join(d, name), "wb") as fh:
            fh.write(G.file_bytes(GCASES, name))
    for cid, data in GFILES.items():
        with open(os.path.join(d, BY_ID[cid]["output"]), "wb") as fh:
            fh.write(data)
    for name, text in CASES["files"].items():
        with open(os.path.join(d, name), "wb") as fh:
            fh.write(text.encode("latin-1"))
    for name, rec in CASES["lists"].items():
        write_list(os.path.join(d, name + ".list"), make_records(np.array([w for w, _ in rec], dtype=np.uint64), np.array([c for _, c in rec], dtype=np.uint32)), LIST_K)
    for cid in CASES["built"] if built else ():
        c = BY_ID[cid]
        if built == "model":
            import index_model as IM
            with open(os.path.join(d, c["output"]), "wb") as fh:
                fh.write(IM.index_bytes([G.file_bytes(GCASES, n) for n in c["inputs"]], c["inputs"], c["k"]))
        else:
            p = subprocess.run([gmaker_util.BINARY] + c["argv"], cwd=d, capture_output=True, timeout=300)
            assert p.returncode == 0, p.stderr
    return d


def run(argv, cwd, hide_gpu=False, env=None):
    e = dict(os.environ)
    if hide_gpu:
        e.update(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    e.update(env or {})
    return subprocess.run([BINARY] + argv, cwd=cwd, capture_output=True, env=e, timeout=300)
