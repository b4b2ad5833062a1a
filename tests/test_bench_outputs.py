"""bench.py --dump-outputs without a GPU: which records are sampled, and the files they are written to.  The GPU suite runs
the option end to end (tests/test_multi_gpu.py)."""
import os
import subprocess
import sys

import numpy as np

import bench
from genometester4_amd.listio import make_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_sample_is_fixed_distinct_and_ascending():
    assert np.array_equal(bench.dump_sample(5, 8), np.arange(5))
    a, b = bench.dump_sample(2_000_000_000, bench.DUMP_RECORDS), bench.dump_sample(2_000_000_000, bench.DUMP_RECORDS)
    assert np.array_equal(a, b) and len(a) == bench.DUMP_RECORDS
    assert (np.diff(a) > 0).all() and a[0] >= 0 and a[-1] < 2_000_000_000


def test_written_arrays_are_float64_exact_and_within_64_mb(tmp_path):
    n = bench.DUMP_RECORDS
    keys = np.sort(np.random.default_rng(3).integers(0, (1 << 64) - 1, size=n, dtype=np.uint64, endpoint=True)) | np.uint64(1 << 63)  # 64-bit keys
    counts = np.random.default_rng(4).integers(1, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    idx = bench.dump_sample(10 * n, n)
    bench.write_dump(str(tmp_path), "intrsec", 10 * n, (1 << 64) - 1, idx, make_records(keys, counts))
    files = sorted(os.listdir(tmp_path))
    assert files == sorted("intrsec_%s.npy" % w for w in ("totals", "index", "key_hi", "key_lo", "count"))
    assert sum(os.path.getsize(os.path.join(tmp_path, f)) for f in files) <= 64 << 20
    d = {f[len("intrsec_"):-len(".npy")]: np.load(os.path.join(tmp_path, f)) for f in files}
    assert all(a.dtype == np.float64 for a in d.values())
    assert d["totals"][0] == 10 * n and np.array_equal(d["index"], idx.astype(np.float64))
    back = (d["key_hi"].astype(np.uint64) << np.uint64(32)) | d["key_lo"].astype(np.uint64)
    assert np.array_equal(back, keys) and np.array_equal(d["count"].astype(np.uint32), counts)


def test_dump_outputs_is_refused_where_there_is_no_pair_output():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "sort", "--dump-outputs", "x"],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 2 and "pair workloads" in p.stderr and p.stdout == ""
