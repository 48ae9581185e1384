"""Which slices of the headline deck (1024^2 x 4 ppc, tile 16, sort period 128; counted from the head of the box as bench.py
does) re-sort the sheet, and how many of them fall into the windows of `bench.py --steps 20 --warmup 5`."""
import sys, os
sys.path.insert(0, os.getcwd())
from hipace_amd import api, decks
deck = decks.synthetic(1024, 1024, 2)
eng = api.SliceEngine(deck, device=0, tile_size=16, sort_period=128)
eng.begin_step()
at, prev = [], eng.sorts()
for q in range(760):
    eng.solve_slice(1024 - 1 - q)
    s = eng.sorts()
    if s != prev: at.append(q)
    prev = s
print("re-sorts in slices (counted from the head):", at)
print("in the timed window 705..724:", [q for q in at if 705 <= q <= 724], " in the phase window 725..756:", [q for q in at if 725 <= q <= 756])
