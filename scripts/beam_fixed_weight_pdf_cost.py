"""A fixed_weight_pdf beam of N particles into an engine that exists: the device generator, SliceEngine.set_beam_fixed_weight_pdf
(DESIGN 8p), against the host path, decks.fixed_weight_pdf_beam (numpy's generator) + SliceEngine.set_beam_particles (a serial host
loop and an upload), with the same parameters -- the transverse benchmark's driver with u_std = (1, 1, 10) -- on 64^3 cells and on
1024^2 x 1024, N = 10^6 and 10^7.  Host clock around the calls, ending in a device synchronise; median of 3, the two paths
alternating in one session.  (profiles/beam_fixed_weight_pdf.txt).  Usage: python scripts/beam_fixed_weight_pdf_cost.py [file to
write the lines to]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np                                                  # noqa: E402
import torch                                                        # noqa: E402

from hipace_amd import api, decks                                   # noqa: E402

lines = []
for n, nz in ((64, 64), (1024, 1024)):
    deck = dict(decks.synthetic(n, nz, 2), beam_profile=-1)
    eng = api.SliceEngine(deck, tile_size=16, sort_period=128)
    zc, sz = 0.5 * (deck["lo"][2] + deck["hi"][2]), 0.1 * (deck["hi"][2] - deck["lo"][2])
    sx = 0.05 * (deck["hi"][0] - deck["lo"][0])
    pdf, u_std = f"exp(-0.5*((z-{zc!r})/{sz!r})^2)", (1.0, 1.0, 10.0)
    for N in (10 ** 6, 10 ** 7):
        dev, host, gen, kept = [], [], [], {}
        for rep in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            left = eng.set_beam_fixed_weight_pdf(N, pdf, (0.0, 0.0), (sx, sx), u_mean=(0.0, 0.0, 2000.0), u_std=u_std, density=2.0, seed=1)
            eng.sync()
            dev.append(time.perf_counter() - t0)
            kept["device"] = (eng.beam_layout()[0], left)
            t0 = time.perf_counter()
            soa = decks.fixed_weight_pdf_beam(deck, N, 2.0, lambda z: np.exp(-0.5 * ((z - zc) / sz) ** 2), pos_std=(sx, sx),
                                              u_mean=(0.0, 0.0, 2000.0), u_std=u_std, seed=1)
            gen.append(time.perf_counter() - t0)
            out = eng.set_beam_particles(soa, allow_outside=True)
            eng.sync()
            host.append(time.perf_counter() - t0)
            kept["host"] = (eng.beam_layout()[0], (N - soa.shape[1], out))
        lines.append(f"{n} x {n} x {nz}, N = {N:>8d}: device {statistics.median(dev) * 1e3:9.2f} ms (min {min(dev) * 1e3:.2f}, max {max(dev) * 1e3:.2f}; "
                     f"{kept['device'][0]} kept, left out {kept['device'][1]});  host {statistics.median(host) * 1e3:9.1f} ms, of it numpy's draws "
                     f"{statistics.median(gen) * 1e3:.1f} ms ({kept['host'][0]} kept, left out {kept['host'][1]})")
    del eng
print("\n".join(lines))
if len(sys.argv) > 1:      # a file to keep the lines in
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
