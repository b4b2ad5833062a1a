#!/usr/bin/env python3
"""Measurements of gmer_caller on one MI355X -> profiles/caller/ (one JSON line per measurement on stdout).

    library   a set of --train markers resident: milliseconds per gt4hip_caller_mlogl launch (device events, as
              gt4hip_caller_set_last_ms reports them) and per call on the host's clock (launch, 8 bytes back, synchronise);
              the probabilities kernels alone on --call and --kernel-call markers, and the call with its copies
    program   genometester4_amd/gmer_caller file -> /dev/null: a whole training (--no_genotypes), with --slow training and calling, and
              calling alone (--runs 0 --coverage C) on --call markers
    reference the same command lines with --reference PATH (a reference gmer_caller built by the recipe of
              tests/golden/make_golden_caller.py, on the same machine) at --num_threads 16 (its default) and 1

Inputs are seed-built: Poisson counts around a coverage of 30 for genotypes drawn at an allele frequency of 0.3 (the recipe of
tests/caller_util.markers, vectorised).  Every timed library shape is run first untimed; a program run is timed --repeat times after one
run that is thrown away (the reference's trainings, a minute each: once, without that run)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BINARY = os.path.join(ROOT, "genometester4_amd", "gmer_caller")
DEFAULT = (0.0547219, 4.2603e-05, 0.014934, 0.985023, 30.0, 65.48, -0.6792684, 0.3)


def counts(seed, n, coverage=30.0, ploidy=2, maf=0.3):
    rng = np.random.default_rng(seed)
    n_b = rng.binomial(ploidy, maf, size=n)
    n_a = ploidy - n_b
    a = rng.poisson(np.where(n_a > 0, coverage / 2 * n_a, 0.05))
    b = rng.poisson(np.where(n_b > 0, coverage / 2 * n_b, 0.05))
    return a.astype(np.uint32), b.astype(np.uint32)


def table(path, seed, n_auto, n_x, n_y):
    """a marker table as gmer_counter prints it (a female: two copies of X, no Y)"""
    with open(path, "wb") as f:
        for name, n, ploidy, cov in (("%d", n_auto, 2, 30.0), ("X", n_x, 2, 30.0), ("Y", n_y, 2, 0.1)):
            for first in range(0, n, 1 << 20):
                m = min(1 << 20, n - first)
                a, b = counts(seed + first, m, cov, ploidy)
                if name == "X" or name == "Y":
                    rows = ["%s:%d\t2\t%d\t%d" % (name, 1000 + first + i, x, y) for i, (x, y) in enumerate(zip(a.tolist(), b.tolist()))]
                else:
                    rows = ["%d:%d\t2\t%d\t%d" % (1 + (first + i) % 22, 1000 + first + i, x, y) for i, (x, y) in enumerate(zip(a.tolist(), b.tolist()))]
                f.write(("\n".join(rows) + "\n").encode())
                seed += 1


def emit(**kw):
    print(json.dumps(kw), flush=True)


def library(args):
    from genometester4_amd import capi
    ctx = capi.Context(0)
    model = capi.CallerModel(*DEFAULT)
    emit(what="device", info=ctx.device_info())
    a, b = counts(1, args.train)
    s = ctx.caller_set(a, b)
    for _ in range(5):
        s.mlogl(model)
    dev, t0 = [], time.perf_counter()
    for _ in range(args.launches):
        s.mlogl(model)
        dev.append(s.last_ms())
    wall = (time.perf_counter() - t0) * 1e3 / args.launches
    emit(what="mlogl", markers=args.train, launches=args.launches, kernel_ms_median=float(np.median(dev)), kernel_ms_min=min(dev), kernel_ms_max=max(dev),
         call_ms_mean=wall, ns_per_marker=float(np.median(dev)) * 1e6 / args.train)
    s.free()
    for n in (args.call, args.kernel_call):
        a, b = counts(2, n)
        s = ctx.caller_set(a, b)
        for all15 in (False, True):
            if all15 and n > args.call:
                continue
            s.probabilities(model, 0, min(n, 1 << 20), all15=all15)
            t0 = time.perf_counter()
            s.probabilities(model, all15=all15)
            wall = (time.perf_counter() - t0) * 1e3
            emit(what="probabilities", markers=n, all15=all15, kernel_ms=s.last_ms(), call_ms=wall, ns_per_marker=s.last_ms() * 1e6 / n)
        s.free()
    ctx.close()


def timed(cmd, repeat, warm=True):
    if warm:
        subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True)
    out = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True)
        out.append(time.perf_counter() - t0)
    return out


def programs(args):
    d = tempfile.mkdtemp(prefix="gt4caller_bench_")
    train, call = os.path.join(d, "train.txt"), os.path.join(d, "call.txt")
    table(train, 10, args.train, args.train // 10, args.train // 30)
    table(call, 20, args.call, args.call // 20, args.call // 60)
    emit(what="inputs", train_bytes=os.path.getsize(train), call_bytes=os.path.getsize(call))
    runs = [("training", ["--no_genotypes", "--info", train]), ("calling", ["--runs", "0", "--coverage", "30", call])]
    if args.slow:
        runs.insert(1, ("training_and_calling", ["--info", train]))
    for name, argv in runs:
        emit(what="program", which="gmer_caller (this repository)", run=name, seconds=timed([BINARY] + argv, args.repeat))
        if args.reference:
            for threads in ("16", "1"):
                if threads == "1" and name != "calling" and not args.slow:
                    continue  # (a training of 10^5 markers on one thread: minutes)
                emit(what="program", which="reference, --num_threads " + threads, run=name,
                     seconds=timed([args.reference, "--num_threads", threads] + argv, 1 if name != "calling" else args.repeat, warm=name == "calling"))
    for f in (train, call):
        os.remove(f)
    os.rmdir(d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train", type=int, default=100_000)
    ap.add_argument("--call", type=int, default=3_000_000)
    ap.add_argument("--kernel-call", type=int, default=30_000_000)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--reference", default=None)
    ap.add_argument("--slow", action="store_true")
    ap.add_argument("--skip-programs", action="store_true")
    args = ap.parse_args()
    library(args)
    if not args.skip_programs:
        programs(args)


if __name__ == "__main__":
    main()
