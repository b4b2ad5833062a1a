#!/usr/bin/env python3
"""Passes and times of glistcompare --subset (gt4hip_list_subset) on a generated k = 25 list of n records with counts
1 .. max_count (gt4hip_generate), for each of the three methods: SIZE is `fraction` of the items (records, or for rand
occurrences); rand_weighted_unique gets `weighted_fraction` of the records, small enough for its walk to end.

Per method one JSON line: passes ("subset_passes"), subset_us, the wall time of the call, and -- unless --no-cli -- the
wall time of this project's glistcompare on the list written to a file, beside the reference binary's on the same file
when oracle/_ref/glistcompare is there (and whether the two output files are the same bytes).

Usage: tools/subset_bench.py [--n 1e7] [--max-count 8] [--fraction 0.3] [--weighted-fraction 0.05] [--seed 7]
                             [--methods rand rand_unique rand_weighted_unique] [--repeat 2] [--no-cli] [--ref-timeout 600]"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLI = os.path.join(ROOT, "genometester4_amd", "glistcompare")
REF = os.path.join(ROOT, "oracle", "_ref", "glistcompare")
K = 25


def timed_cli(binary, list_file, method, size, seed, where, timeout):
    """(wall seconds or None after the time limit, output bytes or None) of one run in the fresh directory `where`"""
    os.mkdir(where)
    t0 = time.perf_counter()
    try:
        r = subprocess.run([binary, list_file, "--subset", method, str(size), "--seed", str(seed)], cwd=where, capture_output=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        shutil.rmtree(where)
        return None, None
    wall = time.perf_counter() - t0
    out = os.path.join(where, "out_subset_%d.list" % K)
    data = None
    if r.returncode == 0 and os.path.exists(out):
        with open(out, "rb") as f:
            data = f.read()
    else:
        sys.stderr.write("%s: exit %d: %s\n" % (binary, r.returncode, r.stderr.decode()[-300:]))
    shutil.rmtree(where)
    return wall, data


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e7)
    ap.add_argument("--max-count", type=int, default=8)
    ap.add_argument("--fraction", type=float, default=0.3)
    ap.add_argument("--weighted-fraction", type=float, default=0.05)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--methods", nargs="+", default=["rand", "rand_unique", "rand_weighted_unique"])
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--ref-timeout", type=float, default=600)
    args = ap.parse_args()
    from genometester4_amd import capi
    from genometester4_amd.listio import header_bytes
    n = int(args.n)
    methods = {"rand": capi.SUBSET_RAND, "rand_unique": capi.SUBSET_RAND_UNIQUE, "rand_weighted_unique": capi.SUBSET_RAND_WEIGHTED_UNIQUE}
    x0 = ((args.seed & 0xFFFFFFFF) << 16) | 0x330E
    work = tempfile.mkdtemp(prefix="gt4ss_bench_")
    ctx = capi.Context(0)
    try:
        lst = ctx.alloc(n, K)
        ctx.generate(lst, n, 1, args.max_count)
        sum_counts = lst.sum_counts()
        list_file = os.path.join(work, "in.list")
        if not args.no_cli:
            with open(list_file, "wb") as f:
                f.write(header_bytes(K, n, sum_counts))
                f.flush()
                ctx.write_fd(lst, 0, n, f.fileno(), 48)
        for name in args.methods:
            items = sum_counts if name == "rand" else n
            size = int((args.weighted_fraction if name == "rand_weighted_unique" else args.fraction) * items)
            row = dict(method=name, n=n, max_count=args.max_count, items=items, size=size, seed=args.seed)
            for rep in range(args.repeat):
                t0 = time.perf_counter()
                try:
                    n_words, total, out = ctx.subset(lst, methods[name], size, x0)
                except capi.Gt4HipError as e:
                    row["error"] = str(e)
                    break
                row.update(call_ms=round((time.perf_counter() - t0) * 1e3, 3), passes=ctx.get_counter("subset_passes"),
                           subset_us=ctx.get_counter("subset_us"), tile=ctx.get_counter("subset_tile"), n_words=n_words, total_count=total)
                out.free()
            if not args.no_cli and "error" not in row:
                wall, mine = timed_cli(CLI, list_file, name, size, args.seed, os.path.join(work, "run"), args.ref_timeout)
                row["cli_wall_s"] = None if wall is None else round(wall, 3)
                if os.path.exists(REF):
                    wall, ref = timed_cli(REF, list_file, name, size, args.seed, os.path.join(work, "run"), args.ref_timeout)
                    row["ref_wall_s"] = None if wall is None else round(wall, 3)
                    row["same_bytes"] = mine is not None and mine == ref
            print(json.dumps(row), flush=True)
    finally:
        ctx.close()
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
