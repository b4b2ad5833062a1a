#!/usr/bin/env python3
"""gt4hip_sort_pairs against gt4hip_sort_words on the same 1e8 random words of k = 25 (six passes), alternating rounds
after one warm-up round that is also checked: wall time of each call (both allocate their scratch from the pool and
synchronise), and the pair sort's HIP-event time.  Prints one JSON line.  Usage: tools/pair_sort_bench.py"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # the repository root
from genometester4_amd import capi

n, k, rounds = 100_000_000, 25, 6
g = torch.Generator(device="cuda")
g.manual_seed(25)
master = torch.randint(0, 1 << 50, (n,), dtype=torch.int64, device="cuda", generator=g)
vals0 = torch.arange(n, dtype=torch.int64, device="cuda")
ctx = capi.Context(0)
keys_ms, pairs_ms, pairs_kernel_ms = [], [], []
for r in range(rounds + 1):
    w = master.clone()
    torch.cuda.synchronize()
    t = time.perf_counter()
    ctx.sort_words(w.data_ptr(), n, k)
    a = (time.perf_counter() - t) * 1e3
    w2, v = master.clone(), vals0.clone()
    torch.cuda.synchronize()
    t = time.perf_counter()
    ctx.sort_pairs(w2.data_ptr(), v.data_ptr(), n, k)
    b = (time.perf_counter() - t) * 1e3
    if r == 0:
        assert torch.equal(w, w2) and bool((w2[1:] >= w2[:-1]).all()) and torch.equal(master[v], w2)
        continue  # warm-up round: the pool's first allocations
    keys_ms.append(a), pairs_ms.append(b), pairs_kernel_ms.append(ctx.get_counter("sort_us") / 1e3)
ctx.close()
res = dict(n=n, k=k, keys_ms=keys_ms, pairs_ms=pairs_ms, pairs_kernels_ms=pairs_kernel_ms, keys_median=float(np.median(keys_ms)), pairs_median=float(np.median(pairs_ms)),
           ratio=float(np.median(pairs_ms) / np.median(keys_ms)), keys_spread=float((max(keys_ms) - min(keys_ms)) / np.median(keys_ms)))
print(json.dumps(res))
