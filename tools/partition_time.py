#!/usr/bin/env python3
"""The partition launch of the headline pair call, guided against bisected, on one build: counter "partition_us" (HIP events
around the launch) of alternating -i calls with option "part_guided" 0 and -1 on the bench's lists.
Usage: tools/partition_time.py [--n N] [--dist stride|iid|genomic|clustered] [--ops 2] [--reps 7]
Prints one JSON line: the median and the range of partition_us and of the call's device time per option value."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genometester4_amd import capi, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2_000_000_000)
    ap.add_argument("--dist", default="stride")
    ap.add_argument("--ops", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    ctx = capi.Context(0)
    x, y = synth.make_pair(ctx, a.n, 25, a.dist)
    out = {bit: ctx.alloc(max(1, {1: x.n_words + y.n_words, 2: min(x.n_words, y.n_words), 4: x.n_words}[bit]), 25) for bit in (1, 2, 4) if a.ops & bit}
    seen = {0: [], -1: []}
    for rep in range(a.reps + 1):
        for g in (0, -1):
            ctx.set_option("part_guided", g)
            _, _, t = ctx.compare(x, y, a.ops, out=out)
            if rep:  # (the first round warms up)
                seen[g].append((ctx.get_counter("partition_us"), t["device_ms"], t["merge_tiles"]))
    ctx.set_option("part_guided", 0)
    res = {"dist": a.dist, "n": a.n, "ops": a.ops, "tiles": seen[0][0][2]}
    for g, name in ((0, "guided"), (-1, "bisected")):
        us = [s[0] for s in seen[g]]
        res[name] = {"partition_us_median": statistics.median(us), "partition_us_min": min(us), "partition_us_max": max(us),
                     "device_ms_median": round(statistics.median(s[1] for s in seen[g]), 4)}
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
