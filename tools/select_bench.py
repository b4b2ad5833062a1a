#!/usr/bin/env python3
"""Times of glistcompare -u --min_lists M --max_lists X on resident lists (gt4hip_select_multi, gt4hip_select.hip).

The lists are the union bench's (genometester4_amd/synth.py make_lists8: --lists lists of --n entries, --dist stride or iid
keys).  After --warmup calls, the median of --reps (at least 7) of
    (a) union_table     gt4hip_union_table alone: wall time of the call and its own counter "table_us"
    (b) table_select    the select kernels alone (HIP events around them: result.device_ms) on that table as the library
                        built it (ragged for up to 32 lists) and again after gt4hip_table_compact (contiguous), as GB/s over
                        (8 + 4 n_lists) rows + 12 kept bytes; the --count_only form, which stops behind the scan; and, for
                        rows of a multiple of four counts, both ways of reading them (option "select_vec": 16 bytes or a
                        dword per lane)
    (c) select_multi    the whole call (wall time) next to gt4hip_union_multi of the same lists
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lists", type=int, default=8)
    ap.add_argument("--n", type=float, default=5e7, help="entries per list")
    ap.add_argument("--k", type=int, default=25)
    ap.add_argument("--dist", choices=["stride", "iid"], default="stride")
    ap.add_argument("--min_lists", type=int, default=2)
    ap.add_argument("--max_lists", type=int, default=0, help="0: the number of lists")
    ap.add_argument("--cutoff", type=int, default=1)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    assert args.reps >= 7, "the median of at least 7"
    from genometester4_amd import capi, synth
    nl, n = args.lists, int(args.n)
    m, x = args.min_lists, args.max_lists or nl
    ctx = capi.Context(0)
    try:
        lists = synth.make_lists8(ctx, n, args.k, args.dist, nl)
        base = dict(lists=nl, entries_per_list=n, dist=args.dist, k=args.k, min_lists=m, max_lists=x, cutoff=args.cutoff, reps=args.reps,
                    device=ctx.device_info())

        def table_call():
            k = ctx.union_table_device(lists)
            return k, ctx.get_counter("table_us") / 1000.0
        runs = timed(ctx, args.reps, args.warmup, table_call)
        n_keys = runs[0][1][0]
        print(json.dumps(dict(base, what="union_table", rows=n_keys, wall_ms=med([w for w, _ in runs]), table_ms=med([r[1] for _, r in runs]))), flush=True)

        table = ctx.device_table(lists)
        for form in ("as built", "compacted"):
            if form == "compacted":
                if not table.ragged:
                    break
                table.compact()
            for count_only, vec in ((False, 0), (True, 0), (False, -1), (True, -1)):
                if vec and nl % 4:
                    continue  # (such rows are read a dword per lane anyway)
                ctx.set_option("select_vec", vec)

                def select_call():
                    rc, cnt, tot, out = ctx.table_select(table, m, x, args.cutoff, count_only=count_only)
                    if out is not None:
                        out.free()
                    return cnt, tot, ctx.last_multi_device_ms
                runs = timed(ctx, args.reps, args.warmup, select_call)
                kept, total, _ = runs[0][1]
                ms = med([r[2] for _, r in runs])
                moved = (8 + 4 * nl) * n_keys + (0 if count_only else 12 * kept)
                print(json.dumps(dict(base, what="table_select", table="ragged" if table.ragged else "contiguous", form=form, count_only=count_only,
                                      loads="16 bytes per lane" if ctx.get_counter("select_wide") else "a dword per lane", rows=n_keys,
                                      kept=kept, total_count=total, kernels_ms=ms, wall_ms=med([w for w, _ in runs]), bytes=moved,
                                      gb_per_s=round(moved / (ms * 1e-3) / 1e9, 1))), flush=True)
        table.free()
        ctx.set_option("select_vec", 0)

        def whole(fn):
            def call():
                rc, cnt, tot, out = fn()
                out.free()
                return cnt, tot
            return call
        sel = timed(ctx, args.reps, args.warmup, whole(lambda: ctx.select_multi(lists, m, x, args.cutoff)))
        uni = timed(ctx, args.reps, args.warmup, whole(lambda: ctx.union_multi(lists, args.cutoff)))
        s_ms, u_ms = med([w for w, _ in sel]), med([w for w, _ in uni])
        print(json.dumps(dict(base, what="select_multi", kept=sel[0][1][0], total_count=sel[0][1][1], wall_ms=s_ms)), flush=True)
        print(json.dumps(dict(base, what="union_multi", words=uni[0][1][0], total_count=uni[0][1][1], wall_ms=u_ms,
                              one_pass=ctx.get_counter("nway_one_pass"), select_over_union=round(s_ms / u_ms, 3))), flush=True)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
