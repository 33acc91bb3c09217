#!/usr/bin/env python3
"""The distinct kernels of a rocprofv3 --kernel-trace CSV with their call counts, the library's own first: one line per
kernel name with the workgroup size and the distinct grids (in workgroups) it was launched with.
    python3 scripts/kernel_calls.py OUT/run_kernel_trace.csv > profiles/..._kernels.txt"""
import csv
import sys
from collections import Counter, defaultdict


def main():
    calls, wg, grids = Counter(), defaultdict(set), defaultdict(set)
    for path in sys.argv[1:]:
        for r in csv.DictReader(open(path)):
            name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
            calls[name] += 1
            w = int(r["Workgroup_Size_X"])
            wg[name].add(w)
            grids[name].add(int(r["Grid_Size_X"]) // w)
    own = sorted(n for n in calls if n.startswith(("rlnc::", "gf_")))
    for name in own + sorted(n for n in calls if n not in own):
        g = sorted(grids[name])
        shown = ", ".join(map(str, g)) if len(g) <= 8 else "%d .. %d" % (g[0], g[-1])
        threads = "/".join(map(str, sorted(wg[name])))
        print("%6d  %s  [%s threads; workgroups: %s]" % (calls[name], name, threads, shown))


if __name__ == "__main__":
    main()
