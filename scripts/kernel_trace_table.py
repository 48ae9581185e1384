#!/usr/bin/env python3
"""Per-kernel table of a `rocprofv3 --kernel-trace --output-format csv -d DIR` run: calls, total and average duration per
kernel, the launches of one kernel told apart by grid size where they differ (the levels of the multigrid, the two kinds of
k_lower_v3 launch), and the total with and without the runtime's copy / fill kernels.
usage: kernel_trace_table.py DIR [rows]"""
import collections
import csv
import glob
import sys


def main():
    f = glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)[0]
    nrows = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    by = collections.defaultdict(list)
    grids = collections.defaultdict(set)
    for r in csv.DictReader(open(f)):
        name = r["Kernel_Name"]
        g = r.get("Grid_Size_X") or r.get("Grid_Size") or ""
        by[(name, g)].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        grids[name].add(g)
    rows = []
    for (name, g), d in by.items():
        label = name if len(grids[name]) == 1 else f"{name[:44]} grid_x={g}"
        rows.append((label, len(d), sum(d)))
    rows.sort(key=lambda r: -r[2])
    tot = sum(r[2] for r in rows)
    own = sum(r[2] for r in rows if "__amd_rocclr" not in r[0])
    print(f"{'kernel':74s} {'calls':>6s} {'total_us':>12s} {'avg_us':>9s}")
    for label, n, t in rows[:nrows]:
        print(f"{label[:74]:74s} {n:6d} {t:12.1f} {t / n:9.2f}")
    print(f"all kernels {tot / 1e3:.1f} ms; without the runtime's copy and fill kernels {own / 1e3:.1f} ms")


if __name__ == "__main__":
    main()
