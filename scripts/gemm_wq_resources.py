#!/usr/bin/env python3
"""Resource table of the kernels of some csrc files, two source trees side by side.

Compiles the named files of each csrc directory device-only for gfx950 with the Makefile's flags plus
-Rpass-analysis=kernel-resource-usage, reads the compiler's remarks (nothing else), and prints one row per kernel
instantiation: VGPRs, AGPRs, SGPRs, scratch bytes a lane, LDS bytes a block and occupancy, old and new.  Exits 1 if the
sets differ, or scratch, LDS or occupancy of any row does.

The default files are the quantised weight-stream GEMMs (fo_gemm_w8.hip, fo_gemm_w4.hip, fo_gemm_w6.hip), whose
instantiations are matched modulo their fold's renaming (k_w8_xs<14, 4, true> is k_wq_xs<Fp8, 14, 4, true>); --files
names others, matched by name as they are.

--streams also compiles each file with -S and compares every kernel's instruction stream between the trees (labels
normalised, comments and directives dropped; an equality check, it looks for no instruction): one more table of
instruction counts, and exit 1 if a kernel's stream differs -- except the kernels named by --may-differ (matched on
the name before any '<'), which may, but must keep their VGPR count.

    python scripts/gemm_wq_resources.py OLD_CSRC NEW_CSRC > profiles/gemm_wq_fold_resources.txt
    python scripts/gemm_wq_resources.py OLD_CSRC NEW_CSRC --files fo_attn.hip --streams \\
        --may-differ k_relpos_fused,k_relpos_chunks > profiles/relpos_fold_resources.txt
"""
import argparse
import hashlib
import os
import re
import subprocess
import sys

WQ_FILES = ("fo_gemm_w8.hip", "fo_gemm_w4.hip", "fo_gemm_w6.hip")
FLAGS = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -munsafe-fp-atomics -Wno-unused-result".split()
FIELDS = (("VGPRs", "VGPR"), ("AGPRs", "AGPR"), ("TotalSGPRs", "SGPR"), ("ScratchSize [bytes/lane]", "scratch"),
          ("LDS Size [bytes/block]", "LDS"), ("Occupancy [waves/SIMD]", "occ"))
FMT = {"8": "Fp8", "4": "Mxfp4", "6": "Mxfp6"}


def hipcc(csrc, name, *extra):
    cc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    inc = os.path.join(csrc, "..", "..", "include")
    p = subprocess.run([cc, *FLAGS, "-I" + inc, "--cuda-device-only", *extra, os.path.join(csrc, name)],
                       capture_output=True, text=True)
    if p.returncode:
        sys.exit(p.stderr)
    return p


def demangle(sym):
    return subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip()


def canonical(name, f):
    """A demangled kernel name; of the weight-stream GEMM files, in the folded spelling."""
    name = re.sub(r"^void ", "", name)
    name = re.sub(r"\(anonymous namespace\)::", "", name)
    name = re.sub(r"\(.*$", "", name)   # the parameter list
    if f not in WQ_FILES:
        return name
    m = re.match(r"k_w([468])(_qkv|_sk|_xs|_rows)?(<.*>)?$", name)
    if m:
        args = (m.group(3) or "<>")[1:-1]
        return "k_wq%s<%s>" % (m.group(2) or "", ", ".join([FMT[m.group(1)]] + ([args] if args else [])))
    return name.replace("k_w8_rows_merge", "k_wq_rows_merge")


def table(csrc, files):
    rows = {}
    for f in files:
        cur = None
        for line in hipcc(csrc, f, "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull).stderr.splitlines():
            m = re.search(r"remark:\s+(.*?): (.*) \[-Rpass-analysis", line)
            if not m:
                continue
            key, val = m.group(1).strip(), m.group(2).strip()
            if key == "Function Name":
                cur = canonical(demangle(val), f)
                rows[(f, cur)] = {}
            elif cur:
                rows[(f, cur)][key] = val
    return rows


def streams(csrc, files):
    """(file, kernel) -> (instruction count, digest of the stream with labels normalised)."""
    out = {}
    for f in files:
        asm = hipcc(csrc, f, "-S", "-o", "-").stdout
        kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
        cur, ins = None, []
        for line in asm.splitlines():
            m = re.match(r"(\S+):", line)
            if m and m.group(1) in kernels:
                cur, ins = m.group(1), []
            elif cur and re.match(r"\.Lfunc_end\d+:", line):
                out[(f, canonical(demangle(cur), f))] = (len(ins), hashlib.sha256("\n".join(ins).encode()).hexdigest())
                cur = None
            elif cur:
                t = line.split(";")[0].strip()
                if t and not t.startswith(".") and not t.endswith(":"):
                    ins.append(re.sub(r"\.LBB\d+_", ".LBB_", " ".join(t.split())))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--files", default=",".join(WQ_FILES))
    ap.add_argument("--streams", action="store_true")
    ap.add_argument("--may-differ", default="")
    a = ap.parse_args()
    files = a.files.split(",")
    free = set(filter(None, a.may_differ.split(",")))
    old, new = table(a.old, files), table(a.new, files)
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
            if o != n and (short in ("scratch", "LDS", "occ") or (short == "VGPR" and k[1].split("<")[0] in free)):
                bad.append("%s %s: %s %s > %s" % (k[0], k[1], short, o, n))
        print("%-14s %-40s %s" % (k[0], k[1], "  ".join(cells)))
    moved = [k for k in sorted(set(old) & set(new)) if any(old[k][key] != new[k][key] for key, _ in FIELDS)]
    print("\n%d kernels, %d with a figure that moved" % (len(set(old) | set(new)), len(moved)))
    if a.streams:
        so, sn = streams(a.old, files), streams(a.new, files)
        if set(so) != set(old) or set(sn) != set(new):
            bad.append("the assembly and the remarks name different kernels")
        print("\n%-14s %-40s %-24s %s" % ("file", "kernel", "instructions old > new", "stream"))
        for k in sorted(set(so) & set(sn)):
            (co, ho), (cn, hn) = so[k], sn[k]
            same = ho == hn
            print("%-14s %-40s %-24s %s" % (k[0], k[1], co if co == cn else "%d > %d" % (co, cn),
                                            "identical" if same else "differs"))
            if not same and k[1].split("<")[0] not in free:
                bad.append("%s %s: instruction stream differs" % k)
        print("\n%d streams identical, %d differ" % (sum(so[k][1] == sn[k][1] for k in set(so) & set(sn)),
                                                    sum(so[k][1] != sn[k][1] for k in set(so) & set(sn))))
    for b in bad:
        print("FAIL " + b)
    print("verdict: %s" % ("FAIL" if bad else "same instantiations, scratch, LDS and occupancy" +
                           ("; identical instruction streams but for " + ", ".join(sorted(free)) + " (same VGPRs)"
                            if a.streams and free else "; identical instruction streams" if a.streams else "")))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
