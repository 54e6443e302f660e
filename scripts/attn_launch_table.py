#!/usr/bin/env python3
"""Name -> call count of every kernel defined in csrc/fo_attn.hip, from the *_kernel_stats.csv files of one
`rocprofv3 --kernel-trace --stats -f csv -d DIR -- ...` run (all processes of the run summed).  Two builds that pick
the same instantiation for every launch of the same workload print identical tables.

    python scripts/attn_launch_table.py DIR > profiles/attn_fold_launches_new.txt
"""
import csv
import glob
import os
import re
import sys
from collections import Counter

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "freeze-omni_amd", "csrc", "fo_attn.hip")


def main():
    with open(SRC) as f:
        ours = set(re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", f.read()))
    calls = Counter()
    files = glob.glob(os.path.join(sys.argv[1], "**", "*kernel_stats.csv"), recursive=True)
    for path in files:
        with open(path) as f:
            for r in csv.DictReader(f):
                name = re.sub(r"^void |\(anonymous namespace\)::", "", r["Name"])
                name = name[:name.index("(")] if "(" in name else name
                if name.split("<")[0] in ours:
                    calls[name] += int(r["Calls"])
    if not files:
        sys.exit("no *kernel_stats.csv under " + sys.argv[1])
    for name in sorted(calls):
        print("%-40s %d" % (name, calls[name]))
    print("%d instantiations of %d kernels defined in fo_attn.hip, %d launches" %
          (len(calls), len(ours), sum(calls.values())))


if __name__ == "__main__":
    main()
