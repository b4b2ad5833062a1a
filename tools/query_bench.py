#!/usr/bin/env python3
"""Lookups per second of gt4hip_query_lookup against k_level's (glistcompare -mm) on the same lists, same process,
alternating: the planted k = 25 workload of tools/mm_bench.py (|A| = |B| = n), queries = words of A's private part.
Per round and N: the level kernel's probes / device ms (gt4hip_compare_mismatch's own statistics), then the query
kernel's n_queries x V / device ms (gt4hip_query_index_last_ms: kernels only, copies excluded).  Also the statistics
kernels' GB/s over B (12 bytes per record) for comparison with tools/stream_bench.hip's read rate.

Usage: tools/query_bench.py [--n 2e8] [--pa 1e7] [--queries 1e6] [--rounds 3]
Prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=2e8)
    ap.add_argument("--pa", type=float, default=1e7)
    ap.add_argument("--planted", type=float, default=2e5)
    ap.add_argument("--queries", type=float, default=1e6)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    from genometester4_amd import capi
    import mm_bench
    ctx = capi.Context(0)
    try:
        A, B, _ = mm_bench.planted_device_pair(ctx, int(args.n), int(args.pa), int(args.planted))
        rng = np.random.default_rng(5)
        # A's private words: every third residue class, as planted_device_pair lays them out; a sample of A will do
        n_q = int(args.queries)
        first = int(rng.integers(0, max(1, A.n_words - 4 * n_q)))
        words = A.download_range(first, min(4 * n_q, A.n_words - first))["key"][::4][:n_q].copy()
        rng.shuffle(words)
        ix = B.query_index()
        for rnd in range(args.rounds):
            for nmm in (1, 2):
                _, _, t = ctx.compare_mismatch(A, B, capi.OP_DIFF1, nmm, count_only=True)
                ms, probes = t["level_ms"][nmm - 1], t["level_probes"][nmm - 1]
                print(json.dumps(dict(kernel="k_level", round=rnd, n_mm=nmm, words=t["level_words"][nmm - 1], probes=probes, ms=ms,
                                      lookups_per_s=probes / (ms * 1e-3) if ms else None)), flush=True)
                t0 = time.perf_counter()
                val, found = ix.lookup(words, nmm, 0)
                wall = time.perf_counter() - t0
                v = capi.query_variants(25, nmm, 0)
                print(json.dumps(dict(kernel="k_query", round=rnd, n_mm=nmm, queries=len(words), lookups=len(words) * v, ms=ix.last_ms, call_wall_ms=wall * 1e3,
                                      found=int(found.sum()), lookups_per_s=len(words) * v / (ix.last_ms * 1e-3))), flush=True)
        gb = B.n_words * 12 / 1e9
        for name, fn in (("count_stats", lambda: B.count_stats()), ("count_split", lambda: B.count_split(4)), ("count_histogram", lambda: B.count_histogram(16)),
                         ("gc", lambda: B.gc()), ("sum_counts", lambda: B.sum_counts())):
            fn()
            best = 1e9
            for _ in range(3):
                t0 = time.perf_counter()
                fn()
                best = min(best, time.perf_counter() - t0)
            print(json.dumps(dict(kernel=name, records=B.n_words, call_wall_ms=best * 1e3, gb_per_s=gb / best)), flush=True)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
