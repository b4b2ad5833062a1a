#!/usr/bin/env python3
"""gt4hip_text_to_locations against gt4hip_text_to_words on the seeded genome of tests/genome_util.py as FastA (default
10^8 bases, lines of 70, one piece), k = 25, alternating rounds after one warm-up round: the HIP-event span of each call's
extraction kernels (counter "extract_us") and of the radix passes behind it ("sort_us": the keys-only sort of
gt4hip_device_words_to_list, the pair sort of gt4hip_pairs_to_index).  The acceptance condition of DESIGN.md 4.8 is that
the extraction stays below the radix passes of the same call.  Prints one JSON line.  Usage: tools/locations_bench.py [bases]"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import genome_util  # noqa: E402
from genometester4_amd import capi  # noqa: E402

bases, k, rounds = (int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000), 25, 5
codes = genome_util.make_genome(length=bases)
whole = bases // 70 * 70
body = np.empty((whole // 70, 71), dtype=np.uint8)
body[:, :70] = np.frombuffer(b"ACGT", dtype=np.uint8)[codes[:whole]].reshape(-1, 70)
body[:, 70] = 10
text = b">genome\n" + body.tobytes() + np.frombuffer(b"ACGT", dtype=np.uint8)[codes[whole:]].tobytes() + b"\n"
buf = (C.c_char * len(text)).from_buffer_copy(text)
ctx, L = capi.Context(0), capi.lib()
res = dict(bases=bases, k=k, text_bytes=len(text), words_extract_ms=[], words_sort_ms=[], loc_extract_ms=[], loc_sort_ms=[])
for r in range(rounds + 1):
    out, d, n, at = capi.MakerCarry(), C.c_void_p(), C.c_uint64(), C.c_uint64()
    ctx._chk(L.gt4hip_text_to_words(ctx.h, buf, len(text), k, 0, None, C.byref(out), C.byref(d), C.byref(n), C.byref(at)))
    a = ctx.get_counter("extract_us") / 1e3
    lst = ctx.device_words_to_list(d.value, n.value, k)
    b = ctx.get_counter("sort_us") / 1e3
    n_list = lst.n_words
    lst.free()
    L.gt4hip_words_free(ctx.h, d)
    dw, dv, lout, piece = C.c_void_p(), C.c_void_p(), capi.LocationsCarry(), capi.LocationsPiece()
    ctx._chk(L.gt4hip_pairs_reserve(ctx.h, len(text), C.byref(dw), C.byref(dv)))
    ctx._chk(L.gt4hip_text_to_locations(ctx.h, buf, len(text), k, 0, None, C.byref(lout), dw, dv, len(text), C.byref(piece), C.byref(at)))
    c = ctx.get_counter("extract_us") / 1e3
    assert piece.n_words == n.value and piece.n_subseqs == 1 and lout.max_position == bases - k
    ctx.pack_locations(dv.value, piece.n_words, 0, 1, int(lout.max_position).bit_length())
    arrays = capi.IndexArrays()
    ctx._chk(L.gt4hip_pairs_to_index(ctx.h, dw, dv, piece.n_words, k, 1, 0xffffffff, C.byref(arrays)))
    e = ctx.get_counter("sort_us") / 1e3
    assert arrays.n_kmers == n_list and arrays.n_locations == n.value
    L.gt4hip_index_free(ctx.h)
    L.gt4hip_pairs_release(ctx.h)
    if r:
        res["words_extract_ms"].append(a), res["words_sort_ms"].append(b), res["loc_extract_ms"].append(c), res["loc_sort_ms"].append(e)
ctx.close()
for key in ("words_extract_ms", "words_sort_ms", "loc_extract_ms", "loc_sort_ms"):
    res[key.replace("_ms", "_median")] = float(np.median(res[key]))
res["extract_ratio"] = res["loc_extract_median"] / res["words_extract_median"]
res["loc_extract_over_loc_sort"] = res["loc_extract_median"] / res["loc_sort_median"]
print(json.dumps(res))
