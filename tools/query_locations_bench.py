#!/usr/bin/env python3
"""The gather kernel of gt4hip_query_lookup_locations (k_gather_locations), and glistquery --locations end to end.

Default: a synthetic index of 10^8 locations -- 9 x 10^7 words with one location each and one word with 10^7 -- and two
batches that fetch the same 2 x 10^7 locations' worth: UNIT (2 x 10^7 words of one location each) and SKEWED (the word
with 10^7 locations and 10^7 unit words around it).  HIP-event time of the gather kernel alone
(gt4hip_query_index_gather_ms), alternating rounds in one session after a warm-up round each.  The kernel reads 8 bytes
and writes 16 per location (plus 16 bytes of segment table per hit), so it is also stated as 24 bytes x locations / time,
to be set against the copy rate tools/stream_bench prints on the same card in the same session.  Prints one JSON line.

--wall [BASES]: file -> stdout wall time of `glistquery G.index -s reads.fa --locations` (about 10^5 words) on the index
of the seeded genome of tests/genome_util.py (default 10^8 bases, k = 25, built by the drop-in glistmaker --index)
against oracle/_ref/glistquery on the same host, stdout compared byte for byte.

Usage: tools/query_locations_bench.py [--rounds N] | --wall [BASES]"""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from genometester4_amd import capi  # noqa: E402


def kernel_bench(rounds):
    k, n_unit, big, fetch = 16, 90_000_000, 10_000_000, 20_000_000
    n = n_unit + 1
    stride = (1 << (2 * k)) // n
    words = np.arange(n, dtype=np.uint64) * np.uint64(stride) + np.uint64(1)
    at = n // 2                                       # the long word sits in the middle
    counts = np.ones(n, dtype=np.uint64)
    counts[at] = big
    first = np.zeros(n, dtype=np.uint64)
    np.cumsum(counts[:-1], out=first[1:])
    locs = np.arange(n_unit + big, dtype=np.uint64) * np.uint64(2654435761)
    ctx = capi.Context(0)
    ix = capi.LocationIndex(ctx, np.stack([words, first], axis=1), locs, k, (4, 20, 36))
    rng = np.random.default_rng(5)
    unit_ids = np.delete(np.arange(n), at)
    batches = {
        "unit": words[np.sort(rng.choice(unit_ids, size=fetch, replace=False))],
        "skewed": np.concatenate([words[np.sort(rng.choice(unit_ids, size=fetch - big, replace=False))], words[at:at + 1]]),
    }
    batches["skewed"].sort()
    ms = {b: [] for b in batches}
    for r in range(rounds + 1):
        for b, w in batches.items():
            nh, nl, _, _ = ix.lookup_raw(w, canonize=False, hit_capacity=len(w), loc_capacity=fetch, fill=None)
            assert nl == fetch and nh == len(w), (b, nh, nl)
            if r:
                ms[b].append(ix.gather_ms)
    med = {b: float(np.median(v)) for b, v in ms.items()}
    print(json.dumps(dict(index_locations=int(n_unit + big), fetched_locations=fetch, rounds=rounds, gather_ms=ms, median_ms=med,
                          gbytes_per_s={b: 24.0 * fetch / med[b] / 1e6 for b in med}, skewed_over_unit=med["skewed"] / med["unit"],
                          device=str(ctx.device_info()))))
    ix.free()
    ctx.close()


def wall(bases):
    import genome_util
    ours = os.path.join(ROOT, "genometester4_amd", "glistquery")
    maker = os.path.join(ROOT, "genometester4_amd", "glistmaker")
    ref = os.path.join(ROOT, "oracle", "_ref", "glistquery")
    codes = genome_util.make_genome(length=bases)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    whole = bases // 70 * 70
    body = np.empty((whole // 70, 71), dtype=np.uint8)
    body[:, :70] = letters[codes[:whole]].reshape(-1, 70)
    body[:, 70] = 10
    rng = np.random.default_rng(6)
    with tempfile.TemporaryDirectory(prefix="gt4gqloc_wall_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as d:
        with open(os.path.join(d, "genome.fa"), "wb") as fh:
            fh.write(b">genome\n" + body.tobytes() + letters[codes[whole:]].tobytes() + b"\n")
        reads = []
        for r in range(1000):                         # 1000 reads of 125 bases: 101,000 25-mers, every second read reversed
            p = int(rng.integers(0, bases - 125))
            s = letters[codes[p:p + 125]].tobytes().decode()
            reads.append(">r%d\n%s\n" % (r, s if r % 2 else s[::-1].translate(str.maketrans("ACGT", "TGCA"))))
        open(os.path.join(d, "reads.fa"), "w").write("".join(reads))
        t0 = time.perf_counter()
        p = subprocess.run([maker, "genome.fa", "-w", "25", "-o", "G", "--index"], cwd=d, capture_output=True, timeout=900)
        assert p.returncode == 0, p.stderr
        print("glistmaker --index: wall_s %.3f, %d bytes" % (time.perf_counter() - t0, os.path.getsize(os.path.join(d, "G_25.index"))), flush=True)
        argv = ["G_25.index", "-s", "reads.fa", "--locations"]
        outs = []
        for name, binary in (("drop-in", ours), ("drop-in again", ours), ("reference", ref)):
            if not os.path.exists(binary):
                continue
            t0 = time.perf_counter()
            p = subprocess.run([binary] + argv, cwd=d, capture_output=True, timeout=900)
            outs.append(p.stdout)
            print("glistquery -s --locations: %s rc %d wall_s %.3f stdout %d bytes identical %s" % (name, p.returncode, time.perf_counter() - t0, len(p.stdout),
                                                                                                     p.stdout == outs[0]), flush=True)


if __name__ == "__main__":
    if "--wall" in sys.argv:
        i = sys.argv.index("--wall")
        wall(int(float(sys.argv[i + 1])) if len(sys.argv) > i + 1 else 100_000_000)
    else:
        kernel_bench(int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 5)
