"""End-to-end wall time of the drop-in CLI against the reference binary on files in /dev/shm
(GPU box; not part of the product).

    python tools/cli_e2e.py [records_per_list] [--no-ref] [--modes=plain,chunks,gpus2,plain]
    python tools/cli_e2e.py --maker [bases] [--index] [--no-ref] [--keep=DIR]

--maker: glistmaker instead -- the seeded genome of tests/genome_util.py at `bases` (default 10^8) as FastA in /dev/shm,
k = 25, the drop-in (twice: the first run pays the start of the HIP runtime) against oracle/_ref/glistmaker with its
default threads, outputs compared with cmp.  --index: `glistmaker --index` on both sides; the index files may differ in
the four bytes of the file block that the reference leaves undefined (tests/index_model.MASKED), and nowhere else.  --keep=DIR leaves genome.fa in DIR (for a profiler run) and stops there.

Modes of the drop-in: plain (no environment variables: inputs of 4 GiB and more take the chunk pipeline with a
budget the tool chooses, smaller ones stay in one piece), chunks (GT4HIP_HBM_LIMIT: key-range chunks through the
loader / merger / writer pipeline with a quarter of the inputs in flight), gpus2 (two worker processes on the
visible device(s)), and the reference binary.  Prints one line per run and whether the outputs are identical."""
import os, subprocess, sys, time, shutil, tempfile, json
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def maker_main(argv):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import genome_util
    nums = [a for a in argv if a.isdigit()]
    bases = int(nums[0]) if nums else 100_000_000
    keep = [a.split("=", 1)[1] for a in argv if a.startswith("--keep=")]
    index = "--index" in argv
    d = keep[0] if keep else tempfile.mkdtemp(prefix="gt4maker_", dir="/dev/shm")
    os.makedirs(d, exist_ok=True)
    try:
        codes = genome_util.make_genome(length=bases)
        lines = np.frombuffer(b"ACGT", dtype=np.uint8)[codes]
        with open(os.path.join(d, "genome.fa"), "wb") as f:  # lines of 70 bases, as genome_util.fasta_text
            f.write(b">genome seed %d\n" % genome_util.GENOME_SEED)
            whole = len(lines) // 70 * 70
            body = np.empty((whole // 70, 71), dtype=np.uint8)
            body[:, :70] = lines[:whole].reshape(-1, 70)
            body[:, 70] = 10
            f.write(body.tobytes())
            if whole < len(lines):
                f.write(lines[whole:].tobytes() + b"\n")
        print("input: %d bases, %d bytes in %s" % (bases, os.path.getsize(os.path.join(d, "genome.fa")), d), flush=True)
        if keep:
            return
        results = []
        runs = [("ours", os.path.join(ROOT, "genometester4_amd", "glistmaker")), ("ours2", os.path.join(ROOT, "genometester4_amd", "glistmaker"))]
        if "--no-ref" not in argv:
            runs.append(("ref", os.path.join(ROOT, "oracle", "_ref", "glistmaker")))
        for tag, exe in runs:
            t0 = time.perf_counter()
            r = subprocess.run([exe, "genome.fa", "-w", "25", "-o", tag] + (["--index"] if index else []), cwd=d, capture_output=True, env=dict(os.environ, GT4HIP_VERBOSE="1"))
            dt = time.perf_counter() - t0
            print("%-6s rc %d  %.3f s  (%.1f M bases/s)  %s" % (tag, r.returncode, dt, bases / dt / 1e6, r.stderr.decode()[-300:].replace("\n", " | ") if tag != "ref" else ""), flush=True)
            results.append(dict(mode=tag, rc=r.returncode, seconds=dt))
        for tag, _ in runs[1:]:
            if index:  # cmp -l: "<offset from 1> <octal> <octal>" per differing byte; the file block starts at byte 72
                diff = subprocess.run(["cmp", "-l", os.path.join(d, "ours_25.index"), os.path.join(d, tag + "_25.index")], capture_output=True, text=True)
                at = [int(l.split()[0]) - 1 - 72 for l in diff.stdout.split("\n")[:100] if l.strip()]
                same = diff.returncode in (0, 1) and not diff.stderr and set(at) <= {6, 7, 10, 11}
            else:
                same = subprocess.run(["cmp", "-s", os.path.join(d, "ours_25.list"), os.path.join(d, tag + "_25.list")]).returncode == 0
            print("%-6s output identical to ours: %s" % (tag, same), flush=True)
            results.append(dict(mode=tag, identical_to_ours=same))
        print(json.dumps(dict(maker_bases=bases, results=results)))
    finally:
        if not keep:
            shutil.rmtree(d, ignore_errors=True)


if "--maker" in sys.argv:
    maker_main(sys.argv[1:])
    sys.exit(0)

from genometester4_amd import capi
from genometester4_amd.listio import write_list
from bench import build_lists

n = int(sys.argv[1]) if len(sys.argv) > 1 and not sys.argv[1].startswith("-") else 100_000_000
with_ref = "--no-ref" not in sys.argv
d = tempfile.mkdtemp(prefix="gt4cli_", dir="/dev/shm")
results = []
try:
    ctx = capi.Context(0)
    a, b = build_lists(ctx, capi, n, 25, 0)
    for name, lst in (("a", a), ("b", b)):
        fd = os.open(os.path.join(d, name + ".list"), os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        from genometester4_amd.listio import header_bytes
        os.write(fd, header_bytes(25, lst.n_words, lst.sum_counts()))
        ctx.write_fd(lst, 0, lst.n_words, fd, 48)
        os.close(fd)
    ctx.close()
    print("inputs: 2 x %d records (%.1f GB each) in %s, free %.1f GB" % (n, 12 * n / 1e9, d, shutil.disk_usage("/dev/shm").free / 1e9), flush=True)
    ours = os.path.join(ROOT, "genometester4_amd", "glistcompare")
    ref = os.path.join(ROOT, "oracle", "_ref", "glistcompare")
    limit = str(max(64 << 20, 12 * n // 2))  # about a quarter of the inputs in flight
    all_modes = {"plain": (ours, {}), "chunks": (ours, {"GT4HIP_HBM_LIMIT": limit}), "gpus2": (ours, {"GT4HIP_GPUS": "2", "GT4HIP_HBM_LIMIT": limit}),
                 "oneshot": (ours, {"GT4HIP_PIPELINE": "0"}), "ref": (ref, {})}
    all_modes["plain2"] = all_modes["plain"]  # the same again (first-run effects)
    verbose = {"GT4HIP_VERBOSE": "1"} if "--verbose" in sys.argv else {}
    order = [a.split("=", 1)[1] for a in sys.argv if a.startswith("--modes=")]
    order = order[0].split(",") if order else ["plain", "chunks", "gpus2"] + (["ref"] if with_ref else [])
    modes = [(m, all_modes[m][0], all_modes[m][1]) for m in order]
    for tag, exe, env in modes:
        for args in (["-i", "--count_only"], ["-i", "-o", tag], ["-u", "-i", "-d", "-o", tag + "3"]):
            t0 = time.perf_counter()
            r = subprocess.run([exe, "a.list", "b.list"] + args, cwd=d, capture_output=True, env=dict(os.environ, **env, **verbose))
            dt = time.perf_counter() - t0
            print("%-7s %-24s rc %d  %.3f s  (%.1f M k-mers/s)" % (tag, " ".join(args[:-1] if "-o" in args else args), r.returncode, dt, 2 * n / dt / 1e6), flush=True)
            results.append(dict(mode=tag, args=args, rc=r.returncode, seconds=dt, k_mers_per_s=2 * n / dt))
            if r.returncode or verbose:
                print(r.stderr.decode()[-1500:])
        if tag != order[0] and os.path.exists(os.path.join(d, "%s_25_intrsec.list" % order[0])):
            same = all(subprocess.run(["cmp", "-s", os.path.join(d, x % tag), os.path.join(d, x % order[0])]).returncode == 0
                       for x in ("%s_25_intrsec.list", "%s3_25_union.list", "%s3_25_0_diff1.list", "%s3_25_intrsec.list"))
            print("%-7s outputs identical to %s: %s" % (tag, order[0], same), flush=True)
            results.append(dict(mode=tag, identical_to_plain=same))
            for x in ("%s_25_intrsec.list", "%s3_25_union.list", "%s3_25_0_diff1.list", "%s3_25_intrsec.list"):
                os.remove(os.path.join(d, x % tag))
    print(json.dumps(dict(records_per_list=n, results=results)))
finally:
    shutil.rmtree(d, ignore_errors=True)
