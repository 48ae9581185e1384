"""rocprofv3 --kernel-trace sqlite db (scripts/quick_prof.sh leaves it under /tmp/prof_q) -> the kernels of one tile re-sort,
from k_cell_keys to the kernel that writes the launch records, in launch order: mean / min / max duration over the re-sorts
of the run, their sum and the span from the first start to the last end.   usage: python scripts/resort_trace.py <db>"""
import sqlite3, sys
db = sqlite3.connect(sys.argv[1]); cur = db.cursor()
tabs = [r[0] for r in cur.execute("select name from sqlite_master where type='table'")]
kd = [t for t in tabs if t.startswith('rocpd_kernel_dispatch')][0]
ks = [t for t in tabs if t.startswith('rocpd_info_kernel_symbol')][0]
rows = list(cur.execute(f"select s.kernel_name, d.start, d.end from {kd} d join {ks} s on d.kernel_id=s.id order by d.start"))
groups, g = [], None
for name, s, e in rows:
    if "k_cell_keys" in name:
        g = []
    if g is not None:
        g.append((name, s, e))
        if "k_tile_launch_info" in name or "k_tile_launch_order" in name:
            groups.append(g); g = None
print(f"dispatches {len(rows)}; re-sorts {len(groups)}")
if not groups: sys.exit(0)
from collections import Counter
shapes = Counter(tuple(n for n, _, _ in g) for g in groups)
shape = shapes.most_common(1)[0][0]
sel = [g for g in groups if tuple(n for n, _, _ in g) == shape]
print(f"groups with the common kernel sequence: {len(sel)} of {len(groups)}")
tot = 0.0
for i, name in enumerate(shape):
    d = [(g[i][2] - g[i][1])/1e3 for g in sel]
    m = sum(d)/len(d); tot += m
    print(f"{i:2d} {name[:90]:90s} mean_us={m:8.2f} min={min(d):8.2f} max={max(d):8.2f}")
sums = [sum(e - s for _, s, e in g)/1e3 for g in sel]
spans = [(g[-1][2] - g[0][1])/1e3 for g in sel]
print(f"kernel time per re-sort: mean {sum(sums)/len(sums):.2f} us  min {min(sums):.2f}  max {max(sums):.2f}")
print(f"span first start -> last end per re-sort: mean {sum(spans)/len(spans):.2f} us  min {min(spans):.2f}  max {max(spans):.2f}")
