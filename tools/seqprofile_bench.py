#!/usr/bin/env python3
"""Rates of glistquery --per_sequence: the kernel k_seq_profile (gt4hip_seqprofile.hip), one gt4hip_query_profile_text
call taken apart, and the command line from a file to stdout.

Kernel (default): a list of --kmers (3e7) random canonical 25-mers and --words (1e8) device-resident words, 0.1 % ("miss")
or all ("hit") of them words of the list, with raw locations of three shapes: reads of 100 words, one single sequence,
one-word sequences.  HIP-event time of the call's kernels (gt4hip_query_index_last_ms: k_seq_zero + k_seq_profile<true>).
The yardstick is gt4hip_gmer_count_words (k_gmer_count, gt4hip_gmer_db_last_ms) on the SAME device words and the same keys
in the same round: the same probe without the 8 more bytes per word and without the sums per sequence.  --rounds alternating
rounds after a warm-up round; the table gives the median and the spread (min .. max) and the ratio of the medians.
Call (--call): a seeded FastQ text of --call-reads reads in host memory through gt4hip_query_profile_text as one piece: wall
time of the call, the reader's kernels (counter "extract_us"), the lookups and sums (last_ms), the rest (copies in, the
read-backs, allocation); with -mm 1 on a smaller text, and gt4hip_query_lookup of the same words for k_query's share.
Command line (--cli): a FastQ file of --reads reads of 101 bases of a random genome and the list of every other 25-mer of it
in --dir (default /dev/shm); wall time of `glistquery LIST -s READS --per_sequence > out`, twice.  --ref BINARY times the
reference's `glistquery LIST -s READS -min 1 > out` on the same files on THIS host (its per-k-mer output is the only way to the
same answer there; it needs no GPU, --no-gpu skips the rest) and checks that the lines per read and their sums ARE the
drop-in's output when both ran.  Every measurement is one JSON line on stdout; --out DIR also writes them to DIR/results.jsonl
and a table to DIR/TABLE.md."""
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
RESULTS = []


def emit(**kw):
    RESULTS.append(kw)
    print(json.dumps(kw), flush=True)


def canonical(w, k=K):
    x, r = ~w, np.zeros_like(w)
    for _ in range(k):
        r = (r << np.uint64(2)) | (x & np.uint64(3))
        x = x >> np.uint64(2)
    return np.minimum(w, r)


def kernel_bench(args):
    import torch
    from genometester4_amd import capi
    from genometester4_amd.listio import make_records
    rng = np.random.default_rng(args.seed)
    n_db, n = int(args.kmers), int(args.words)
    canon = np.unique(canonical(rng.integers(0, 1 << (2 * K), size=n_db + n_db // 16, dtype=np.uint64)))
    canon = np.sort(canon[rng.permutation(len(canon))[:n_db]])
    counts = rng.integers(1, 100, size=n_db, dtype=np.uint32)
    ctx = capi.Context(0)
    try:
        emit(what="device", device=ctx.device_info(), kmers=n_db, words=n, profile_tile=ctx.get_counter("profile_tile"))
        ix = ctx.upload(make_records(canon, counts), K).query_index()
        db = ctx.gmer_db(canon, K)
        d_canon = torch.from_numpy(canon.view(np.int64)).cuda()
        d_counts = torch.from_numpy(counts.astype(np.int64)).cuda()
        g = torch.Generator(device="cuda").manual_seed(args.seed)
        batches, expect = {}, {}
        miss = torch.randint(0, 1 << (2 * K), (n,), dtype=torch.int64, device="cuda", generator=g)
        at = torch.arange(0, n, 1000, device="cuda")
        pick = torch.randint(0, n_db, (len(at),), device="cuda", generator=g)
        miss[at] = d_canon[pick]
        batches["miss"] = miss
        pick_hit = torch.randint(0, n_db, (n,), device="cuda", generator=g)
        batches["hit"] = d_canon[pick_hit]
        expect["hit"] = (n, int(d_counts[pick_hit].sum().item()))
        i = torch.arange(n, dtype=torch.int64, device="cuda")
        shapes = {"reads": ((i // 100) << 33, (n + 99) // 100), "single": (torch.zeros_like(i), 1), "one-word": (i << 33, n)}
        del i, pick_hit
        torch.cuda.synchronize()
        for r in range(args.rounds + 1):  # round 0 warms up
            for name, words in batches.items():
                db.reset()
                hits, _ = db.count_words(words.data_ptr(), capi.GMER_ON_DEVICE, n)
                ms = db.last_ms()
                if r:
                    emit(what="k_gmer_count", batch=name, round=r, words=n, hits=hits, ms=round(ms, 4))
                for shape, (raw, n_seqs) in shapes.items():
                    t0 = time.time()
                    prof = ctx.query_profile_words(ix, words.data_ptr(), raw.data_ptr(), n, 0, n_seqs)
                    wall = time.time() - t0
                    ms = ix.last_ms
                    got = (int(prof["n_words"].sum()), int(prof["n_hits"].sum()), int(prof["sum"].sum()))
                    assert got[0] == n and got[1] == hits, (name, shape, got, hits)  # (a random word is a list word now and then)
                    assert name != "hit" or got[1:] == expect["hit"], (got, expect)
                    del prof
                    if r:
                        emit(what="k_seq_profile", batch=name, shape=shape, round=r, words=n, sequences=n_seqs, hits=got[1], ms=round(ms, 4), call_wall_s=round(wall, 3))
        ix.free()
        db.free()
    finally:
        ctx.close()


def fastq_bytes(rng, genome, n_reads, lo=0, L=101, name_w=10):
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    starts = rng.integers(0, len(genome) - L, size=n_reads)
    rec = np.empty((n_reads, 1 + name_w + 1 + L + 3 + L + 1), dtype=np.uint8)
    rec[:, 0] = ord("@")
    digits = np.arange(lo, lo + n_reads)
    for c in range(name_w):
        rec[:, name_w - c] = ord("0") + digits % 10
        digits //= 10
    rec[:, 1 + name_w] = 10
    rec[:, 2 + name_w:2 + name_w + L] = letters[genome[starts[:, None] + np.arange(L)[None, :]]]
    rec[:, 2 + name_w + L:5 + name_w + L] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rec[:, 5 + name_w + L:5 + name_w + 2 * L] = ord("I")
    rec[:, -1] = 10
    return rec


def genome_list(genome):
    """(keys, counts): every other 25-mer of the genome, canonical, with the number of times it was taken"""
    codes = genome.astype(np.uint64)
    at = np.arange(0, len(genome) - K, 2)
    w = np.zeros(len(at), dtype=np.uint64)
    for j in range(K):
        w = (w << np.uint64(2)) | codes[at + j]
    keys, counts = np.unique(canonical(w), return_counts=True)
    return keys, counts.astype(np.uint32)


def call_bench(args):
    from genometester4_amd import capi
    from genometester4_amd.listio import make_records
    rng = np.random.default_rng(args.seed)
    genome = rng.integers(0, 4, size=int(args.genome), dtype=np.uint8)
    keys, counts = genome_list(genome)
    ctx = capi.Context(0)
    try:
        ix = ctx.upload(make_records(keys, counts), K).query_index()
        for mm, n_reads in ((0, int(args.call_reads)), (1, int(args.call_reads) // 16)):
            text = fastq_bytes(rng, genome, n_reads).tobytes()
            for r in range(args.rounds + 1):
                prof, _ = ctx.query_profile_text(ix, [text], mm, capacity=n_reads)
                wall = ctx.profile_call_s
                if r:
                    emit(what="profile_text", mm=mm, round=r, bytes=len(text), sequences=len(prof), words=int(prof["n_words"].sum()), hits=int(prof["n_hits"].sum()),
                         wall_ms=round(wall * 1e3, 3), reader_ms=round(ctx.get_counter("extract_us") / 1e3, 3), lookups_and_sums_ms=round(ix.last_ms, 3))
            if mm:
                words, _ = ctx.text_to_words(text, K)
                for r in range(args.rounds + 1):
                    ix.lookup(words, mm)
                    if r:
                        emit(what="query_lookup", mm=mm, round=r, words=len(words), k_query_ms=round(ix.last_ms, 3))
        ix.free()
    finally:
        ctx.close()


def cli_bench(args):
    from genometester4_amd.listio import make_records, write_list
    rng = np.random.default_rng(args.seed)
    genome = rng.integers(0, 4, size=int(args.genome), dtype=np.uint8)
    keys, counts = genome_list(genome)
    lst, reads = os.path.join(args.dir, "seqprofile_bench.list"), os.path.join(args.dir, "seqprofile_bench_reads.fq")
    write_list(lst, make_records(keys, counts), K)
    n_reads = int(args.reads)
    with open(reads, "wb") as f:
        for lo in range(0, n_reads, 1 << 17):  # in blocks: the index matrix of a block is 100 MB
            fastq_bytes(rng, genome, min(1 << 17, n_reads - lo), lo).tofile(f)
    sizes = dict(reads=n_reads, reads_bytes=os.path.getsize(reads), list_words=len(keys))
    out, ref_out = os.path.join(args.dir, "seqprofile_bench_out.txt"), os.path.join(args.dir, "seqprofile_bench_ref.txt")
    try:
        if not args.no_gpu:
            for run in (1, 2):
                t0 = time.time()
                with open(out, "wb") as f:
                    p = subprocess.run([os.path.join(ROOT, "genometester4_amd", "glistquery"), lst, "-s", reads, "--per_sequence"], stdout=f, stderr=subprocess.PIPE)
                assert p.returncode == 0, p.stderr
                emit(what="cli", binary="drop-in", run=run, wall_s=round(time.time() - t0, 3), stdout_bytes=os.path.getsize(out), **sizes)
        if args.ref:
            t0 = time.time()
            with open(ref_out, "wb") as f:
                p = subprocess.run([args.ref, lst, "-s", reads, "-min", "1"], stdout=f, stderr=subprocess.PIPE)
            assert p.returncode == 0, p.stderr
            emit(what="cli", binary="reference", host_cpus=os.cpu_count(), wall_s=round(time.time() - t0, 3), stdout_bytes=os.path.getsize(ref_out), **sizes)
            hits = total = 0
            with open(ref_out, "rb") as f:  # WORD<TAB>VALUE lines, a block of whole lines at a time
                rest = b""
                while True:
                    block = f.read(1 << 26)
                    block, rest = (rest + block).rsplit(b"\n", 1) if block else (rest, b"")
                    v = np.array(block.split()[1::2], dtype=np.uint64)
                    hits, total = hits + len(v), total + int(v.sum())
                    if not block and not rest:
                        break
            emit(what="reference_totals", hits=hits, sum=total)
            if os.path.exists(out):
                got = np.loadtxt(out, dtype=np.uint64, usecols=(1, 2, 3), ndmin=2)
                assert (int(got[:, 1].sum()), int(got[:, 2].sum())) == (hits, total), "the drop-in's sums are not the reference's lines"
    finally:
        for f in (lst, reads, out, ref_out):
            if os.path.exists(f):
                os.remove(f)


def table():
    """the medians per measurement as markdown"""
    def med(rows, key):
        v = sorted(r[key] for r in rows)
        return v[len(v) // 2], v[0], v[-1]

    lines = []
    dev = [r for r in RESULTS if r["what"] == "device"]
    if dev:
        lines += ["Device: `%s`; %d k-mers in the list, %d words per batch, tiles of %d words." % (dev[0]["device"], dev[0]["kmers"], dev[0]["words"], dev[0]["profile_tile"]), ""]
    prof = [r for r in RESULTS if r["what"] == "k_seq_profile"]
    if prof:
        lines += ["| batch | shape | sequences | kernels ms (min .. max) | words/s | k_gmer_count ms (min .. max) | ratio |", "|---|---|---|---|---|---|---|"]
        for batch in ("miss", "hit"):
            y = med([r for r in RESULTS if r["what"] == "k_gmer_count" and r["batch"] == batch], "ms")
            for shape in ("reads", "single", "one-word"):
                rows = [r for r in prof if r["batch"] == batch and r["shape"] == shape]
                m = med(rows, "ms")
                lines.append("| %s | %s | %d | %.3f (%.3f .. %.3f) | %.3g | %.3f (%.3f .. %.3f) | %.2f |" % (batch, shape, rows[0]["sequences"], m[0], m[1], m[2],
                                                                                                       rows[0]["words"] / (m[0] * 1e-3), y[0], y[1], y[2], m[0] / y[0]))
        lines.append("")
    for mm in (0, 1):
        rows = [r for r in RESULTS if r["what"] == "profile_text" and r["mm"] == mm]
        if rows:
            w, rd, ks = med(rows, "wall_ms")[0], med(rows, "reader_ms")[0], med(rows, "lookups_and_sums_ms")[0]
            line = "gt4hip_query_profile_text, -mm %d, %d bytes, %d words in %d reads: call %.2f ms = reader %.2f (%.0f %%) + lookups and sums %.2f (%.0f %%) + copies, read-backs, allocation %.2f (%.0f %%)." % (
                mm, rows[0]["bytes"], rows[0]["words"], rows[0]["sequences"], w, rd, 100 * rd / w, ks, 100 * ks / w, w - rd - ks, 100 * (w - rd - ks) / w)
            q = [r for r in RESULTS if r["what"] == "query_lookup" and r["mm"] == mm]
            if q:
                line += "  gt4hip_query_lookup of the same words: k_query %.2f ms, %.0f %% of the lookups and sums." % (med(q, "k_query_ms")[0], 100 * med(q, "k_query_ms")[0] / ks)
            lines += [line, ""]
    for r in RESULTS:
        if r["what"] == "cli":
            lines.append("Command line, %s, run %s: %.3f s for %d reads, %d bytes of FastQ, a list of %d words; %d bytes of output." % (
                r["binary"], r.get("run", 1), r["wall_s"], r["reads"], r["reads_bytes"], r["list_words"], r["stdout_bytes"]))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kmers", type=float, default=3e7)
    ap.add_argument("--words", type=float, default=1e8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--call", action="store_true")
    ap.add_argument("--call-reads", type=float, default=5e5)
    ap.add_argument("--cli", action="store_true")
    ap.add_argument("--no-gpu", action="store_true")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--ref", default=None)
    ap.add_argument("--reads", type=float, default=2e6)
    ap.add_argument("--genome", type=float, default=5e6)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not args.no_gpu and not args.no_kernel:
        kernel_bench(args)
    if args.call and not args.no_gpu:
        call_bench(args)
    if args.cli or args.ref:
        cli_bench(args)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "results.jsonl"), "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in RESULTS)
        with open(os.path.join(args.out, "TABLE.md"), "w") as f:
            f.write(table())


if __name__ == "__main__":
    main()
