#!/usr/bin/env python3
"""Is the device code of two trees the same, kernel by kernel, wherever a kernel lives?
Usage: tools/device_asm_diff.py OTHER_TREE [THIS_TREE]

Every .hip of <tree>/genometester4_amd/csrc is compiled with the command its Makefile would run for it (make -n), with
-S --offload-device-only in place of -c.  For every kernel (.amdhsa_kernel NAME) the text from its label to its
.end_amdhsa_kernel is compared between the trees; lines that name __hip_cuid_* (a fresh random symbol per compile) are
dropped, and so is the number of the function inside its file in the assembler's local labels (.LBB<n>_, .Lfunc_end<n>)
and in its loop comments (BB<n>_), which changes when a kernel moves to another file or is instantiated in another order.  Files present in both trees are compared whole as they are.  Exit status 0: every kernel of either tree is in the
other with the same text."""
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def device_asm(csrc, source, tmp):
    """the device assembly of csrc/<source> under the Makefile's own flags for it, without the __hip_cuid_ lines"""
    plan = subprocess.run(["make", "-n", "-B", "-C", csrc, source + ".o"], capture_output=True, text=True, check=True).stdout
    cmd = next(ln for ln in plan.split("\n") if " -c " + source in ln).split()
    i = cmd.index("-c")
    out = os.path.join(tmp, source + ".s")
    cmd[i:] = ["-S", "--offload-device-only", source, "-o", out]
    subprocess.run(cmd, cwd=csrc, check=True, capture_output=True)
    return [ln for ln in open(out).read().split("\n") if "__hip_cuid_" not in ln]


def kernels(lines):
    """{name: text from the kernel's label to its .end_amdhsa_kernel}"""
    label = {m.group(1): i for i, m in enumerate(re.match(r"([A-Za-z_$][\w$.]*):", ln) for ln in lines) if m}
    found = {}
    for i, ln in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            end = next(j for j in range(i, len(lines)) if ".end_amdhsa_kernel" in lines[j])
            text = re.sub(r"(\.LBB|\.Lfunc_begin|\.Lfunc_end|\bBB)\d+", r"\1", "\n".join(lines[label[m.group(1)]:end + 1]))
            found[m.group(1)] = re.sub(r"[ \t]+;", " ;", text)   # comments are aligned to a column: a shorter number, other padding
    return found


def tree(root):
    csrc = os.path.join(root, "genometester4_amd", "csrc")
    sources = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(8) as ex:
        return dict(zip(sources, ex.map(lambda s: device_asm(csrc, s, tmp), sources)))


def main():
    other, this = sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else HERE
    a, b = tree(other), tree(this)
    ka = {n: (f, t) for f, lines in a.items() for n, t in kernels(lines).items()}
    kb = {n: (f, t) for f, lines in b.items() for n, t in kernels(lines).items()}
    bad = 0
    for f in sorted(set(a) | set(b)):
        na, nb = sum(x[0] == f for x in ka.values()), sum(x[0] == f for x in kb.values())
        whole = "-" if f not in a or f not in b else ("identical" if a[f] == b[f] else "DIFFERENT")
        print("%-22s kernels %3d -> %3d   whole file: %s" % (f, na, nb, whole))
    for n in sorted(set(ka) | set(kb)):
        if n not in ka or n not in kb:
            print("ONLY IN %s: %s" % ("OTHER" if n in ka else "THIS", n))
            bad += 1
        elif ka[n][1] != kb[n][1]:
            print("BODY DIFFERS: %s (%s -> %s)" % (n, ka[n][0], kb[n][0]))
            bad += 1
        elif ka[n][0] != kb[n][0]:
            print("moved, identical: %s (%s -> %s)" % (n, ka[n][0], kb[n][0]))
    print("%d kernels in the other tree, %d in this one, %d differ or are missing" % (len(ka), len(kb), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
