#!/usr/bin/env python3
"""Resource table of the quantised weight-stream GEMM kernels, two source trees side by side.

Compiles fo_gemm_w8.hip, fo_gemm_w4.hip and fo_gemm_w6.hip of each csrc directory device-only for gfx950 with the
Makefile's flags plus -Rpass-analysis=kernel-resource-usage, reads the compiler's remarks (nothing else), and prints
one row per kernel instantiation: VGPRs, AGPRs, SGPRs, scratch bytes a lane, LDS bytes a block and occupancy, old and
new.  Instantiations are matched modulo the fold's renaming (k_w8_xs<14, 4, true> is k_wq_xs<Fp8, 14, 4, true>).
Exits 1 if the sets differ, or scratch, LDS or occupancy of any row does.

    python scripts/gemm_wq_resources.py OLD_CSRC NEW_CSRC > profiles/gemm_wq_fold_resources.txt
"""
import os
import re
import subprocess
import sys

FILES = ("fo_gemm_w8.hip", "fo_gemm_w4.hip", "fo_gemm_w6.hip")
FLAGS = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -munsafe-fp-atomics -Wno-unused-result".split()
FIELDS = (("VGPRs", "VGPR"), ("AGPRs", "AGPR"), ("TotalSGPRs", "SGPR"), ("ScratchSize [bytes/lane]", "scratch"),
          ("LDS Size [bytes/block]", "LDS"), ("Occupancy [waves/SIMD]", "occ"))
FMT = {"8": "Fp8", "4": "Mxfp4", "6": "Mxfp6"}


def remarks(csrc, name):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    inc = os.path.join(csrc, "..", "..", "include")
    p = subprocess.run([hipcc, *FLAGS, "-I" + inc, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(csrc, name), "-o", os.devnull], capture_output=True, text=True)
    if p.returncode:
        sys.exit(p.stderr)
    return p.stderr


def canonical(name):
    """A demangled kernel name in the folded spelling."""
    name = re.sub(r"^void ", "", name)
    name = re.sub(r"\(anonymous namespace\)::", "", name)
    name = re.sub(r"\(.*$", "", name)   # the parameter list
    m = re.match(r"k_w([468])(_qkv|_sk|_xs|_rows)?(<.*>)?$", name)
    if m:
        args = (m.group(3) or "<>")[1:-1]
        return "k_wq%s<%s>" % (m.group(2) or "", ", ".join([FMT[m.group(1)]] + ([args] if args else [])))
    return name.replace("k_w8_rows_merge", "k_wq_rows_merge")


def table(csrc):
    rows = {}
    for f in FILES:
        cur = None
        for line in remarks(csrc, f).splitlines():
            m = re.search(r"remark:\s+(.*?): (.*) \[-Rpass-analysis", line)
            if not m:
                continue
            key, val = m.group(1).strip(), m.group(2).strip()
            if key == "Function Name":
                cur = canonical(subprocess.run(["c++filt", val], capture_output=True, text=True).stdout.strip())
                rows[(f, cur)] = {}
            elif cur:
                rows[(f, cur)][key] = val
    return rows


def main():
    old, new = table(sys.argv[1]), table(sys.argv[2])
    bad = []
    print("%-14s %-40s %s" % ("file", "kernel", "  ".join("%-11s" % s for _, s in FIELDS)))
    print("%-14s %-40s %s" % ("", "", "  ".join("%-11s" % "old > new" for _ in FIELDS)))
    for k in sorted(set(old) | set(new)):
        if k not in old or k not in new:
            bad.append("%s %s: only in the %s tree" % (k[0], k[1], "old" if k in old else "new"))
            continue
        cells = []
        for key, short in FIELDS:
            o, n = old[k][key], new[k][key]
            cells.append("%-11s" % (o if o == n else "%s > %s" % (o, n)))
            if o != n and short in ("scratch", "LDS", "occ"):
                bad.append("%s %s: %s %s > %s" % (k[0], k[1], short, o, n))
        print("%-14s %-40s %s" % (k[0], k[1], "  ".join(cells)))
    moved = [k for k in sorted(set(old) & set(new)) if any(old[k][key] != new[k][key] for key, _ in FIELDS)]
    print("\n%d kernels, %d with a figure that moved" % (len(set(old) | set(new)), len(moved)))
    for b in bad:
        print("FAIL " + b)
    print("verdict: %s" % ("FAIL" if bad else "same instantiations, scratch, LDS and occupancy"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
