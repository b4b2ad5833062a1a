#!/usr/bin/env python3
"""Rates of gmer_counter's counting kernel (k_gmer_count, gt4hip_gmer.hip) and wall time of the command line.

Kernel: a synthetic database of --kmers (default 3e7) random canonical 25-mers, and --words (default 2^27) device-resident
words per batch; HIP-event time of the kernel alone (gt4hip_gmer_db_last_ms), --rounds alternating rounds after a warm-up,
each batch in both forms of the hit atomics (default: a wavefront whose hits all fall on one k-mer adds them with one
atomic; GMER_PLAIN_ATOMICS: one atomic per hit):
    miss      about 0.1 % of the words are database k-mers (every 1000th), the rest random words
    hit       every word is a database k-mer, drawn at random: the 64 of a wavefront are different ones
    hot       every word is the SAME database k-mer (a read of one repeated base)
Command line (--cli): a seeded FastQ file of --reads reads of 101 bases cut out of a random genome and a text database of
--nodes nodes with two 25-mers of that genome each, written to --dir (default /dev/shm); wall time of
`gmer_counter -db DB --stats --total READS > out`, twice (the first run pays the cold start of the HIP runtime).
--ref BINARY times the reference's gmer_counter on the same two files on THIS host (it needs no GPU; --no-gpu skips the rest)
and compares the outputs byte for byte.  Prints one JSON line per measurement."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K = 25


def canonical(w, k=K):
    x, r = ~w, np.zeros_like(w)
    for _ in range(k):
        r = (r << np.uint64(2)) | (x & np.uint64(3))
        x = x >> np.uint64(2)
    return np.minimum(w, r)


def kernel_bench(args):
    import torch
    from genometester4_amd import capi
    rng = np.random.default_rng(args.seed)
    n_db, n = int(args.kmers), int(args.words)
    canon = np.unique(canonical(rng.integers(0, 1 << (2 * K), size=n_db + n_db // 16, dtype=np.uint64)))
    canon = canon[rng.permutation(len(canon))[:n_db]]
    ctx = capi.Context(0)
    try:
        t0 = time.time()
        db = ctx.gmer_db(canon, K)
        print(json.dumps(dict(what="db_create", kmers=n_db, wall_s=round(time.time() - t0, 3), device=ctx.device_info())), flush=True)
        d_canon = torch.from_numpy(canon.view(np.int64)).cuda()
        g = torch.Generator(device="cuda").manual_seed(args.seed)
        batches = {}
        miss = torch.randint(0, 1 << (2 * K), (n,), dtype=torch.int64, device="cuda", generator=g)
        at = torch.arange(0, n, 1000, device="cuda")
        miss[at] = d_canon[torch.randint(0, n_db, (len(at),), device="cuda", generator=g)]
        batches["miss"] = miss
        batches["hit"] = d_canon[torch.randint(0, n_db, (n,), device="cuda", generator=g)]
        batches["hot"] = d_canon[12345 % n_db].repeat(n)
        torch.cuda.synchronize()
        forms = dict(combine=0, plain=capi.GMER_PLAIN_ATOMICS)
        expect = {}
        for r in range(args.rounds + 1):  # round 0 warms up
            for name, words in batches.items():
                for form, flag in forms.items():
                    db.reset()
                    hits, gc = db.count_words(words.data_ptr(), capi.GMER_ON_DEVICE | flag, n)
                    assert expect.setdefault(name, (hits, gc)) == (hits, gc), (name, form)
                    ms = db.last_ms()
                    if r:
                        print(json.dumps(dict(what="k_gmer_count", batch=name, atomics=form, round=r, words=n, hits=hits, ms=round(ms, 4),
                                              words_per_s=float("%.4g" % (n / (ms * 1e-3))))), flush=True)
        assert expect["hit"][0] == n and expect["hot"][0] == n and abs(expect["miss"][0] - len(at)) <= 64  # (a random word is a database k-mer now and then)
        db.free()
    finally:
        ctx.close()


def write_inputs(args):
    rng = np.random.default_rng(args.seed)
    n_reads, L = int(args.reads), 101
    genome = rng.integers(0, 4, size=int(args.genome), dtype=np.uint8)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    name_w = 10
    reads = os.path.join(args.dir, "gmer_bench_reads.fq")
    with open(reads, "wb") as f:
        for lo in range(0, n_reads, 1 << 17):  # in blocks: the index matrix of a block is 100 MB
            m = min(1 << 17, n_reads - lo)
            starts = rng.integers(0, len(genome) - L, size=m)
            rec = np.empty((m, 1 + name_w + 1 + L + 3 + L + 1), dtype=np.uint8)
            rec[:, 0] = ord("@")
            digits = np.arange(lo, lo + m)
            for c in range(name_w):
                rec[:, name_w - c] = ord("0") + digits % 10
                digits //= 10
            rec[:, 1 + name_w] = 10
            rec[:, 2 + name_w:2 + name_w + L] = letters[genome[starts[:, None] + np.arange(L)[None, :]]]
            rec[:, 2 + name_w + L:5 + name_w + L] = np.frombuffer(b"\n+\n", dtype=np.uint8)
            rec[:, 5 + name_w + L:5 + name_w + 2 * L] = ord("I")
            rec[:, -1] = 10
            rec.tofile(f)
    n_nodes = int(args.nodes)
    at = rng.permutation(len(genome) - K)[:2 * n_nodes]
    kmers = letters[genome[at[:, None] + np.arange(K)[None, :]]]
    codes = genome[at[:, None] + np.arange(K)[None, :]].astype(np.uint64)
    w = np.zeros(len(at), dtype=np.uint64)
    for j in range(K):
        w = (w << np.uint64(2)) | codes[:, j]
    _, first = np.unique(canonical(w), return_index=True)
    keep = np.sort(first)
    keep = keep[:len(keep) // 2 * 2]
    db = os.path.join(args.dir, "gmer_bench_db.txt")
    with open(db, "wb") as f:
        f.write(b"# gmer_bench: seed %d, %d nodes of two 25-mers\n" % (args.seed, len(keep) // 2))
        for i in range(0, len(keep), 2):
            f.write(b"n%d\t2\t%s\t%s\n" % (i // 2, kmers[keep[i]].tobytes(), kmers[keep[i + 1]].tobytes()))
    return db, reads


def timed(binary, db, reads, out):
    t0 = time.time()
    with open(out, "wb") as f:
        p = subprocess.run([binary, "-db", db, "--stats", "--total", reads], stdout=f, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr
    return time.time() - t0


def cli_bench(args):
    db, reads = write_inputs(args)
    sizes = dict(reads_bytes=os.path.getsize(reads), db_bytes=os.path.getsize(db))
    outs = {}
    if not args.no_gpu:
        binary = os.path.join(ROOT, "genometester4_amd", "gmer_counter")
        for run in (1, 2):
            outs["dropin"] = os.path.join(args.dir, "gmer_bench_out.txt")
            print(json.dumps(dict(what="cli", binary="drop-in", run=run, wall_s=round(timed(binary, db, reads, outs["dropin"]), 3), **sizes)), flush=True)
    if args.ref:
        outs["ref"] = os.path.join(args.dir, "gmer_bench_ref.txt")
        print(json.dumps(dict(what="cli", binary="reference", host=os.uname().nodename, cpus=os.cpu_count(),
                              wall_s=round(timed(args.ref, db, reads, outs["ref"]), 3), **sizes)), flush=True)
    import hashlib
    print(json.dumps(dict(what="cli_outputs", sha256={k: hashlib.sha256(open(v, "rb").read()).hexdigest() for k, v in outs.items()})), flush=True)
    for f in [db, reads] + list(outs.values()):
        os.remove(f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kmers", type=float, default=3e7)
    ap.add_argument("--words", type=float, default=float(1 << 27))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--cli", action="store_true")
    ap.add_argument("--no-gpu", action="store_true")
    ap.add_argument("--ref", default=None)
    ap.add_argument("--reads", type=float, default=2e6)
    ap.add_argument("--genome", type=float, default=5e6)
    ap.add_argument("--nodes", type=float, default=5e5)
    ap.add_argument("--dir", default="/dev/shm")
    args = ap.parse_args()
    if not args.no_gpu:
        kernel_bench(args)
    if args.cli or args.ref:
        cli_bench(args)


if __name__ == "__main__":
    main()
