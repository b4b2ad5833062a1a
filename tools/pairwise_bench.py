#!/usr/bin/env python3
"""Times of glistcompare L1 .. LN --pairwise on resident lists (gt4hip_pairwise_multi, gt4hip_pairwise.hip).

The lists are the union bench's (genometester4_amd/synth.py make_lists8: --lists lists of --n entries, --dist stride or iid
keys), or with --collection a collection: --lists lists over one universe of --n iid words, of which a core (--core of 330
parts) lies in every list and the rest in one, two or three lists in equal parts.  After --warmup calls, the median of --reps
(at least 7) of
    (a) union_table      gt4hip_union_table alone (wall time of the call)
    (b) table_pairwise   the pairwise kernels alone (HIP events around them: device_ms) on that table as the library built
                         it (ragged for up to 32 lists) and again after gt4hip_table_compact (contiguous), as GB/s over the
                         table's counts, 4 n_lists bytes per row
    (c) pairwise_multi   the whole call (wall time)
    (d) compare_loop     the baseline: gt4hip_compare, intersection, --count_only, over all n (n - 1) / 2 pairs of the same
                         resident lists (wall time of the loop); checked against the matrices of (c)
Prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(ctx, reps, warmup, fn):
    """[(wall ms, what fn returned)] of `reps` calls behind `warmup` calls"""
    out = []
    for it in range(warmup + reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        r = fn()
        ctx.synchronize()
        if it >= warmup:
            out.append(((time.perf_counter() - t0) * 1e3, r))
    return out


def med(xs):
    return round(statistics.median(xs), 4)


def collection(ctx, synth, n_lists, words, k, core):
    """classes of words: `core` classes every list holds, then per list one class of its own, one it shares with the next
    list and one it shares with the next two"""
    member = []
    for j in range(n_lists):
        m = list(range(core)) + [core + j]
        m += [core + n_lists + (j - d) % n_lists for d in range(2)]
        m += [core + 2 * n_lists + (j - d) % n_lists for d in range(3)]
        member.append(tuple(m))
    return synth._from_universe(ctx, "iid", words, k, core + 3 * n_lists, member, 4444)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lists", type=int, default=8)
    ap.add_argument("--n", type=float, default=5e7, help="entries per list (--collection: words of the universe)")
    ap.add_argument("--k", type=int, default=25)
    ap.add_argument("--dist", choices=["stride", "iid"], default="stride")
    ap.add_argument("--collection", action="store_true")
    ap.add_argument("--core", type=int, default=30, help="--collection: classes of words, of core + 3 x lists, that every list holds")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop_reps", type=int, default=0, help="repetitions of the baseline loop (0: as --reps)")
    args = ap.parse_args()
    assert args.reps >= 7, "the median of at least 7"
    from genometester4_amd import capi, synth
    nl, n = args.lists, int(args.n)
    ctx = capi.Context(0)
    try:
        lists = collection(ctx, synth, nl, n, args.k, args.core) if args.collection else synth.make_lists8(ctx, n, args.k, args.dist, nl)
        records = sum(l.n_words for l in lists)
        base = dict(lists=nl, dist="collection" if args.collection else args.dist, k=args.k, records=records, reps=args.reps, device=ctx.device_info())

        def table_call():
            return ctx.union_table_device(lists)
        runs = timed(ctx, args.reps, args.warmup, table_call)
        print(json.dumps(dict(base, what="union_table", rows=runs[0][1], wall_ms=med([w for w, _ in runs]))), flush=True)

        table = ctx.device_table(lists)
        rows = table.n_keys
        for form in ("as built", "compacted"):
            if form == "compacted":
                if not table.ragged:
                    break
                table.compact()

            def kernels_call():
                shared, min_total = ctx.table_pairwise(table)
                return int(shared.sum()), ctx.last_pairwise_ms
            runs = timed(ctx, args.reps, args.warmup, kernels_call)
            ms = med([r[1] for _, r in runs])
            passes = (nl + 31) // 32
            print(json.dumps(dict(base, what="table_pairwise", table="ragged" if table.ragged else "contiguous", form=form, rows=rows,
                                  kernels_ms=ms, wall_ms=med([w for w, _ in runs]), table_bytes=4 * nl * rows, times_read=passes,
                                  gb_per_s=round(4 * nl * rows / (ms * 1e-3) / 1e9, 1))), flush=True)
        table.free()

        runs = timed(ctx, args.reps, args.warmup, lambda: ctx.pairwise_multi(lists))
        shared, min_total = runs[0][1]
        mean_holders = float(shared.diagonal().sum()) / max(rows, 1)
        print(json.dumps(dict(base, what="pairwise_multi", rows=rows, lists_per_row=round(mean_holders, 3), wall_ms=med([w for w, _ in runs]))), flush=True)

        def loop():
            out = {}
            for i in range(nl):
                for j in range(i + 1, nl):
                    out[i, j] = ctx.compare(lists[i], lists[j], capi.OP_INTRSEC, count_only=True)[0][capi.OP_INTRSEC]
            return out
        runs = timed(ctx, args.loop_reps or args.reps, 1, loop)
        for (i, j), (words, total) in runs[0][1].items():
            assert (words, total) == (int(shared[i][j]), int(min_total[i][j])), (i, j)
        print(json.dumps(dict(base, what="compare_loop", pairs=nl * (nl - 1) // 2, reps=args.loop_reps or args.reps, wall_ms=med([w for w, _ in runs]))), flush=True)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
