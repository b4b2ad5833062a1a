#!/usr/bin/env python3
"""Device times of glistcompare -mm N (gt4hip_compare_mismatch) on the planted k = 25 workload of DESIGN.md section 5:
A = S + PA and B = S + PB + planted from disjoint residue classes (gt4hip_generate_ex, three classes, as bench.py),
|A| = |B| = n, |PA| = |PB| = n_pa, and one-mismatch neighbours of `n_planted` words of PA (canonical) merged into B.
The pre-pass table is PA; -mm 1 drops the planted words, -mm 2 runs on the rest.

Usage: tools/mm_bench.py [--n 2e8] [--pa 1e7] [--planted 2e5] [--levels 1 2] [--repeat 2]
Prints one JSON line per (N, repeat): pre-pass ms, per-level ms / words / probes, probes per second."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def planted_device_pair(ctx, n, n_pa, n_planted, k=25, seed=77):
    """(A, B, planted source words) as device lists; see the module doc"""
    from genometester4_amd import capi
    from genometester4_amd.listio import make_records
    import mismatch_util as MU
    rng = np.random.default_rng(seed)
    S, PA, PB = ctx.alloc(n - n_pa, k), ctx.alloc(n_pa, k), ctx.alloc(n_pa, k)
    ctx.generate_ex(S, n - n_pa, 1, 2, 8, 3, 0)
    ctx.generate_ex(PA, n_pa, 3, 4, 8, 3, 1)
    ctx.generate_ex(PB, n_pa, 5, 6, 8, 3, 2)
    A = ctx.alloc(n, k)
    ctx.compare(S, PA, capi.OP_UNION, out={1: A})
    pa = PA.download()["key"]
    src = np.sort(pa[rng.choice(len(pa), n_planted, replace=False)])
    pos = rng.integers(0, k, size=len(src)).astype(np.uint64)
    sub = rng.integers(1, 4, size=len(src)).astype(np.uint64)
    var = np.unique(MU.canonical(src ^ (sub << (np.uint64(2) * pos)), k))
    P = ctx.upload(make_records(var, np.ones(len(var), dtype=np.uint32)), k)
    SB = ctx.alloc(n, k)
    ctx.compare(S, PB, capi.OP_UNION, out={1: SB})
    B = ctx.alloc(n + len(var), k)
    ctx.compare(SB, P, capi.OP_UNION, out={1: B})
    for x in (S, PA, PB, SB, P):
        x.free()
    return A, B, src


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=2e8)
    ap.add_argument("--pa", type=float, default=1e7)
    ap.add_argument("--planted", type=float, default=2e5)
    ap.add_argument("--levels", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--repeat", type=int, default=2)
    args = ap.parse_args()
    from genometester4_amd import capi
    ctx = capi.Context(0)
    try:
        A, B, _ = planted_device_pair(ctx, int(args.n), int(args.pa), int(args.planted))
        for nmm in args.levels:
            for rep in range(args.repeat):
                st, out, t = ctx.compare_mismatch(A, B, capi.OP_DIFF1, nmm, count_only=True)
                level_probes = t["level_probes"]
                print(json.dumps(dict(n=int(args.n), n_pa=int(args.pa), planted=int(args.planted), n_mismatch=nmm, rep=rep,
                                      out_words=st[4][0], prepass_ms=round(t["prepass_ms"], 3), prepass_words=t["prepass_words"][0],
                                      level_ms=[round(x, 3) for x in t["level_ms"]], level_words=t["level_words"],
                                      level_probes=level_probes, device_ms=round(t["device_ms"], 3),
                                      level_probes_per_s=[round(p / (ms * 1e-3)) if ms else 0 for p, ms in zip(level_probes, t["level_ms"])])),
                      flush=True)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
