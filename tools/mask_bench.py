#!/usr/bin/env python3
"""Rates of glistquery --mask: the two kernels of gt4hip_mask.hip, one gt4hip_query_mask_text call beside its neighbours,
and the command line from a file to stdout.

A genome of --kmers (3e7) random bases; the list holds every 25-mer of it.  Texts of --bytes (1e8) bytes in device memory:
"fasta" (records of 10^4 lines of 60 columns) and "fastq" (reads of 150 bases), each "hit" (cut from the genome: every
word is a word of the list) and "miss" (random bases with 100 words of the genome in every 10^5: 0.1 %).  Per text, after two
warm-ups, the median of --rounds (7) of:

    mask     gt4hip_query_mask_text, text and masked text on the device: wall time of the call, the reader's kernels (counter
             "extract_us"), the lookups with k_mask_ends ("mask_ends_us") and k_mask_apply ("mask_apply_us")
    copy     a device-to-device copy of the same bytes (HIP events): 1 B read and 1 B written per byte, k_mask_apply's floor
    gmer     gt4hip_gmer_count_text on the same text, a database of the same k-mers, no statistics: the same reader and probe
             without the masking
    profile  gt4hip_query_profile_text on the same text and index: the reader with locations, and the sums per sequence

Command line (--cli): a FastQ file of --cli-bytes (2e8) bytes in --dir and the list; wall time of
`glistquery LIST -s READS --mask > out`, twice.  Every measurement is one JSON line on stdout; --out DIR also writes them
to DIR/results.jsonl and a table to DIR/TABLE.md."""
import argparse
import ctypes as C
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
LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)


def emit(**kw):
    RESULTS.append(kw)
    print(json.dumps(kw), flush=True)


def canonical(w, k=K):
    x, r = ~w, np.zeros_like(w)
    for _ in range(k):
        r = (r << np.uint64(2)) | (x & np.uint64(3))
        x = x >> np.uint64(2)
    return np.minimum(w, r)


def genome_words(genome):
    """the canonical 25-mers of the genome, sorted, each once"""
    codes = genome.astype(np.uint64)
    n = len(genome) - K + 1
    w = np.zeros(n, dtype=np.uint64)
    for j in range(K):
        w = (w << np.uint64(2)) | codes[j:j + n]
    return np.unique(canonical(w))


def source(rng, genome, n_bases, hit):
    """n_bases codes: stretches of the genome (hit), or random codes with 124 bases of the genome in every 10^5 (miss)"""
    if hit:
        return np.resize(genome, n_bases)
    out = rng.integers(0, 4, size=n_bases, dtype=np.uint8)
    for at in range(0, n_bases - 124, 100_000):
        s = int(rng.integers(0, len(genome) - 124))
        out[at:at + 124] = genome[s:s + 124]
    return out


def fasta_text(rng, genome, n_bytes, hit):
    lines = n_bytes // 61
    body = np.empty((lines, 61), dtype=np.uint8)
    body[:, :60] = LETTERS[source(rng, genome, lines * 60, hit)].reshape(lines, 60)
    body[:, 60] = 10
    parts = []
    for i in range(0, lines, 10_000):
        parts += [b">s%07d\n" % i, body[i:i + 10_000].tobytes()]
    return b"".join(parts)


def fastq_text(rng, genome, n_bytes, hit, L=150, name_w=10):
    n = n_bytes // (2 * L + name_w + 6)
    rec = np.empty((n, 2 * L + name_w + 6), dtype=np.uint8)
    rec[:, 0] = ord("@")
    digits = np.arange(n)
    for c in range(name_w):
        rec[:, name_w - c] = ord("0") + digits % 10
        digits //= 10
    rec[:, 1 + name_w] = 10
    rec[:, 2 + name_w:2 + name_w + L] = LETTERS[source(rng, genome, n * L, hit)].reshape(n, L)
    rec[:, 2 + name_w + L:5 + name_w + L] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rec[:, 5 + name_w + L:5 + name_w + 2 * L] = ord("I")
    rec[:, -1] = 10
    return rec.tobytes()


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def device_bench(args):
    import torch
    from genometester4_amd import capi
    from genometester4_amd.listio import make_records
    rng = np.random.default_rng(args.seed)
    genome = rng.integers(0, 4, size=int(args.kmers), dtype=np.uint8)
    keys = genome_words(genome)
    counts = rng.integers(1, 100, size=len(keys), dtype=np.uint32)
    L = capi.lib()
    ctx = capi.Context(0)
    try:
        emit(what="device", device=ctx.device_info(), kmers=len(keys), bytes=int(args.bytes), tile=ctx.get_counter("maker_text_tile"))
        ix = ctx.upload(make_records(keys, counts), K).query_index()
        db = ctx.gmer_db(keys, K)
        prm = capi.QueryParams(0, 0, 1)
        for kind, make in (("fasta", fasta_text), ("fastq", fastq_text)):
            for hit in (False, True):
                text = make(rng, genome, int(args.bytes), hit)
                n = len(text)
                d_text = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
                d_out = torch.empty_like(d_text)
                n_seqs = text.count(b">" if kind == "fasta" else b"\n@") + 1
                prof = np.empty(n_seqs + 1, dtype=capi.SEQ_PROFILE_DTYPE)
                rows = dict(mask=[], ends=[], apply=[], reader=[], copy=[], gmer=[], profile=[])
                words = hits = covered = 0
                for r in range(args.rounds + 2):  # two warm-ups
                    out, piece, err = capi.MakerCarry(), capi.MaskPiece(), C.c_uint64()
                    t0 = time.perf_counter()
                    rc = L.gt4hip_query_mask_text(ctx.h, ix.h, C.c_void_p(d_text.data_ptr()), n, capi.MAKER_TEXT_ON_DEVICE, C.byref(prm), 1, 0xFFFFFFFF, ord("N"), None,
                                                  C.byref(out), C.c_void_p(d_out.data_ptr()), C.byref(piece), C.byref(err))
                    t_mask = time.perf_counter() - t0
                    assert rc == 0, L.gt4hip_last_error(ctx.h)
                    words, hits, covered = piece.n_words, piece.n_hits, piece.n_covered
                    ends_ms, apply_ms, reader_ms = ctx.get_counter("mask_ends_us") / 1e3, ctx.get_counter("mask_apply_us") / 1e3, ctx.get_counter("extract_us") / 1e3
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    d_out.copy_(d_text)
                    e1.record()
                    torch.cuda.synchronize()
                    copy_ms = e0.elapsed_time(e1)
                    out2 = capi.MakerCarry()
                    t0 = time.perf_counter()
                    rc = L.gt4hip_gmer_count_text(ctx.h, db.h, C.c_void_p(d_text.data_ptr()), n, capi.GMER_ON_DEVICE, None, C.byref(out2), None, C.byref(err))
                    t_gmer = time.perf_counter() - t0
                    assert rc == 0, L.gt4hip_last_error(ctx.h)
                    out3, lp, n_prof = capi.LocationsCarry(), capi.LocationsPiece(), C.c_uint64()
                    t0 = time.perf_counter()
                    rc = L.gt4hip_query_profile_text(ctx.h, ix.h, C.c_void_p(d_text.data_ptr()), n, capi.MAKER_TEXT_ON_DEVICE, C.byref(prm), 1, 0xFFFFFFFF, None, C.byref(out3),
                                                     C.byref(lp), prof.ctypes.data, len(prof), C.byref(n_prof), C.byref(err))
                    t_prof = time.perf_counter() - t0
                    assert rc == 0 and n_prof.value <= len(prof), (rc, n_prof.value, L.gt4hip_last_error(ctx.h))
                    assert int(prof["n_hits"][:n_prof.value].sum()) == hits and int(prof["n_words"][:n_prof.value].sum()) == words
                    L.gt4hip_locations_free(ctx.h)
                    if r >= 2:
                        for key, v in (("mask", t_mask * 1e3), ("ends", ends_ms), ("apply", apply_ms), ("reader", reader_ms), ("copy", copy_ms), ("gmer", t_gmer * 1e3),
                                       ("profile", t_prof * 1e3)):
                            rows[key].append(v)
                assert hits > words - 1000 if hit else hits < words // 500  # (a word across the end of the genome, where a stretch wraps, is no word of it)
                emit(what="call", kind=kind, batch="hit" if hit else "miss", bytes=n, words=words, hits=hits, covered=covered,
                     **{key + "_ms": round(median(v), 4) for key, v in rows.items()}, **{key + "_ms_min_max": [round(min(v), 4), round(max(v), 4)] for key, v in rows.items()})
                del d_text, d_out
        ix.free()
        db.free()
    finally:
        ctx.close()


def cli_bench(args):
    from genometester4_amd.listio import make_records, write_list
    rng = np.random.default_rng(args.seed)
    genome = rng.integers(0, 4, size=int(args.kmers), dtype=np.uint8)
    keys = genome_words(genome)
    lst, reads, out = (os.path.join(args.dir, "mask_bench" + s) for s in (".list", "_reads.fq", "_out.fq"))
    write_list(lst, make_records(keys, rng.integers(1, 100, size=len(keys), dtype=np.uint32)), K)
    with open(reads, "wb") as f:
        f.write(fastq_text(rng, genome, int(args.cli_bytes), True))
    try:
        for run in (1, 2):
            t0 = time.time()
            with open(out, "wb") as f:
                p = subprocess.run([os.path.join(ROOT, "genometester4_amd", "glistquery"), lst, "-s", reads, "--mask"], stdout=f, stderr=subprocess.PIPE)
            assert p.returncode == 0, p.stderr
            assert os.path.getsize(out) == os.path.getsize(reads)
            emit(what="cli", run=run, wall_s=round(time.time() - t0, 3), bytes=os.path.getsize(reads), list_words=len(keys))
    finally:
        for f in (lst, reads, out):
            if os.path.exists(f):
                os.remove(f)


def table():
    lines = []
    dev = [r for r in RESULTS if r["what"] == "device"]
    if dev:
        lines += ["Device: `%s`; a list of %d 25-mers; texts of %d bytes; tiles of %d bytes." % (dev[0]["device"], dev[0]["kmers"], dev[0]["bytes"], dev[0]["tile"]), ""]
    calls = [r for r in RESULTS if r["what"] == "call"]
    if calls:
        lines += ["| text | words | hits | lookups + k_mask_ends ms | k_mask_apply ms | copy ms | apply / copy | reader ms | mask_text ms | gmer_count_text ms | profile_text ms | mask / gmer | mask / profile |",
                  "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for r in calls:
            lines.append("| %s %s | %d | %d | %.3f | %.3f | %.3f | %.2f | %.3f | %.2f | %.2f | %.2f | %.2f | %.2f |" % (
                r["kind"], r["batch"], r["words"], r["hits"], r["ends_ms"], r["apply_ms"], r["copy_ms"], r["apply_ms"] / r["copy_ms"], r["reader_ms"], r["mask_ms"],
                r["gmer_ms"], r["profile_ms"], r["mask_ms"] / r["gmer_ms"], r["mask_ms"] / r["profile_ms"]))
        lines.append("")
    for r in RESULTS:
        if r["what"] == "cli":
            lines.append("Command line, run %d: %.3f s for %d bytes of FastQ to stdout, a list of %d words." % (r["run"], r["wall_s"], r["bytes"], r["list_words"]))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kmers", type=float, default=3e7)
    ap.add_argument("--bytes", type=float, default=1e8)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--cli", action="store_true")
    ap.add_argument("--cli-bytes", type=float, default=2e8)
    ap.add_argument("--no-device", action="store_true")
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not args.no_device:
        device_bench(args)
    if args.cli:
        cli_bench(args)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "results.jsonl"), "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in RESULTS)
        with open(os.path.join(args.out, "TABLE.md"), "w") as f:
            f.write(table())


if __name__ == "__main__":
    main()
