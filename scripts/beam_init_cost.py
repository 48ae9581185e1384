"""SliceEngine(deck) to a usable beam at the headline shape (1024^2 x 1024 cells, the bench's beam window, 1 x 1 x 1 per cell):
the host loop of Engine::init_beam against the device generator of hps_engine_set_beam_fixed_ppc, for the flat-top
beam (a constant program) and for the Gaussian (decks.beam_profile_expr), next to the same deck without a beam.  Host clock
around the constructor, ending in a device synchronise; median of 5, the five cases alternating in one session; the device
cases also clock the setter alone.  The first round compares the flat-top beams of the two paths bit for bit on the device.
(profiles/beam_init.txt).  Usage: python scripts/beam_init_cost.py [file to write the lines to]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch                                                        # noqa: E402

from hipace_amd import api, decks                                   # noqa: E402

base = decks.synthetic(1024, 1024, 2)


def with_program(deck):
    text, constants = decks.beam_profile_expr(deck)
    d = dict(deck, **decks.BEAM_INIT_DEFAULT)
    d.update(beam_density_expr=text, beam_density_constants=constants)
    return d


flat, gauss = dict(base, beam_profile=1), dict(base, beam_profile=0)
cases = {
    "no beam": dict(base, beam_profile=-1),
    "flat top, host loop": flat,
    "flat top, device": with_program(flat),
    "gaussian, host loop": gauss,
    "gaussian, device": with_program(gauss),
}


def blocks(eng):
    n, _ = eng.beam_layout()
    t = torch.zeros(7 * n, dtype=torch.float64, device="cuda")
    eng.initial_beam_into(t)
    return t


times, setter, counts, notes = {k: [] for k in cases}, {k: [] for k in cases}, {}, []
for rep in range(5):
    kept = {}
    for name, deck in cases.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng = api.SliceEngine(deck, tile_size=16, sort_period=128)
        eng.sync()
        times[name].append(time.perf_counter() - t0)
        if "device" in name:      # the setter alone, on the engine that has its beam already
            spec = decks.beam_init(deck)
            t0 = time.perf_counter()
            eng.set_beam_fixed_ppc(**spec)
            eng.sync()
            setter[name].append(time.perf_counter() - t0)
        counts[name] = eng.beam_layout()[0]
        if rep == 0 and name.startswith("flat top"):
            kept[name] = blocks(eng)
        del eng
    if rep == 0:
        a, b = kept["flat top, host loop"], kept["flat top, device"]
        notes.append(f"flat top, {a.numel() // 7} particles: the device generator's blocks are "
                     f"{'bit-equal to' if torch.equal(a, b) else 'DIFFERENT from'} the host loop's")
    del kept
lines = []
for name, t in times.items():
    s = f"{name:22s} SliceEngine(deck) median {statistics.median(t):7.3f} s  min {min(t):7.3f}  max {max(t):7.3f}  (n = {len(t)}, {counts[name]} particles)"
    if setter[name]:
        s += f"; set_beam_fixed_ppc alone median {statistics.median(setter[name]) * 1e3:8.2f} ms"
    lines.append(s)
lines += notes
print("\n".join(lines))
if len(sys.argv) > 1:      # a file to keep the lines in
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
