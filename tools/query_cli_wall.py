#!/usr/bin/env python3
"""File -> stdout wall time of the drop-in glistquery against oracle/_ref/glistquery on the same host:

    glistquery L.list -s reads.fa -mm 1 | -mm 2      L: 2 x 10^6 random canonical 25-mers, ~10^5 query k-mers
    glistquery M.list --median                       M: --median-records records (default 2 x 10^8)

Outputs are compared byte for byte.  Usage: tools/query_cli_wall.py [--median-records N] [--no-ref-mm2]
Prints one line per run."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from genometester4_amd.listio import header_bytes, make_records, write_list  # noqa: E402
import query_model as M  # noqa: E402

OURS = os.path.join(ROOT, "genometester4_amd", "glistquery")
REF = os.path.join(ROOT, "oracle", "_ref", "glistquery")


def timed(argv, cwd, timeout):
    t0 = time.perf_counter()
    p = subprocess.run(argv, cwd=cwd, capture_output=True, timeout=timeout)
    return time.perf_counter() - t0, p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--median-records", type=float, default=2e8)
    ap.add_argument("--no-ref-mm2", action="store_true")
    args = ap.parse_args()
    rng = np.random.default_rng(2025)
    k = 25
    with tempfile.TemporaryDirectory(prefix="gt4gq_wall_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as d:
        keys = np.unique(M.canonical_np(rng.integers(0, 1 << 50, size=2_050_000, dtype=np.uint64), k))[:2_000_000]
        write_list(os.path.join(d, "L.list"), make_records(keys, rng.integers(1, 9, size=len(keys), dtype=np.uint32)), k)
        reads = []
        for r in range(1000):  # 1000 reads of 125 bases = 101,000 25-mers, a third of them seeded with a list word
            s = "".join("ACGT"[i] for i in rng.integers(0, 4, size=125))
            if r % 3 == 0:
                w = M.word_to_string(int(keys[int(rng.integers(0, len(keys)))]), k)
                s = s[:40] + w[:12] + "ACGT"[int(rng.integers(0, 4))] + w[13:] + s[65:]
            reads.append(">r%d\n%s\n" % (r, s))
        open(os.path.join(d, "reads.fa"), "w").write("".join(reads))
        for mm in (1, 2):
            argv = ["L.list", "-s", "reads.fa", "-mm", str(mm)]
            t, p = timed([OURS] + argv, d, 600)
            print("glistquery -s -mm %d: drop-in rc %d wall_s %.3f stdout %d bytes" % (mm, p.returncode, t, len(p.stdout)), flush=True)
            if os.path.exists(REF) and not (mm == 2 and args.no_ref_mm2):
                tr, pr = timed([REF] + argv, d, 600)
                print("glistquery -s -mm %d: reference rc %d wall_s %.3f identical %s" % (mm, pr.returncode, tr, pr.stdout == p.stdout), flush=True)
        n = int(args.median_records)
        c = rng.integers(1, 1000, size=n, dtype=np.uint32)
        with open(os.path.join(d, "M.list"), "wb") as f:
            f.write(header_bytes(k, n, int(c.sum(dtype=np.uint64))))
            rec = make_records(np.arange(n, dtype=np.uint64) * np.uint64(5_000_000), c)
            f.write(rec.tobytes())
        del rec
        for cmd in (["--median"], ["--gc"], ["--distribution", "1000"]):
            t, p = timed([OURS, "M.list"] + cmd, d, 600)
            print("glistquery %s (%d records): drop-in rc %d wall_s %.3f" % (" ".join(cmd), n, p.returncode, t), flush=True)
            if os.path.exists(REF):
                tr, pr = timed([REF, "M.list"] + cmd, d, 600)
                print("glistquery %s (%d records): reference rc %d wall_s %.3f identical %s" % (" ".join(cmd), n, pr.returncode, tr, pr.stdout == p.stdout), flush=True)


if __name__ == "__main__":
    main()
