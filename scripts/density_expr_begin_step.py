"""begin_step at the headline shape (1024^2 cells, 2 x 2 particles per cell, tile 16) with the density from the tables, from
the lwfa program and from the depth-16 / 256-instruction program: host clock around begin_step + a device synchronise,
median of 25 steps after 5 warm-up steps, the three cases alternating
(profiles/density_expr.txt).  Usage: python scripts/density_expr_begin_step.py [file to write the lines to]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hipace_amd import api, decks                                   # noqa: E402
from tests.test_density_expr_gpu import deepest_program             # noqa: E402

deck = decks.synthetic(1024, 1024, 2)
lwfa_consts = dict(ne=1.0, kp=1.0, Rm=3.0, Lramp=1.0)               # the file's function in the deck's normalised units; c t = 0.5: on the ramp
cases = {
    "tables": lambda e: None,
    "lwfa program": lambda e: e.set_density_expr(0, decks.LWFA_DENSITY, lwfa_consts),
    "depth-16 program": lambda e: e.set_density_expr(0, deepest_program(), min_density=-1.0e30),
}
engines = {}
for name, setup in cases.items():
    e = api.SliceEngine(deck, tile_size=16, sort_period=128)
    setup(e)
    engines[name] = e
times = {name: [] for name in cases}
for rep in range(30):
    for name, e in engines.items():
        e.set_time(0.5, 0.0)
        e.sync()
        t0 = time.perf_counter()
        e.begin_step()
        e.sync()
        t1 = time.perf_counter()
        if rep >= 5:
            times[name].append((t1 - t0) * 1e3)
lines = []
for name, t in times.items():
    real, valid = engines[name].particles()
    lines.append(f"{name:18s} begin_step median {statistics.median(t):8.3f} ms  min {min(t):8.3f}  max {max(t):8.3f}  (n = {len(t)}, "
                 f"{int((valid != 0).sum())} of {valid.size} slots valid)")
print("\n".join(lines))
if len(sys.argv) > 1:      # a file to keep the lines in
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
