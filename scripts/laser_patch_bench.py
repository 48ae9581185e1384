#!/usr/bin/env python3
"""Rate of BASELINE config 5 with the laser envelope on the field grid (decks.config5) and on a centred patch of its own
(decks.config5_laser_patch): whole boxes through SliceEngine.run_step, a host clock around each box that ends in a device
synchronise, the first box (step 0: Gaussian initialisation, first launches) untimed.  One process per deck, the two decks
alternating --rounds times: with both engines in one process the second one ran at 823 instead of 1195 slices/s (four
streams on a process's four hardware queues; profiles/laser_grid.txt).

    python scripts/laser_patch_bench.py [--n 1024] [--nz 2048] [--n-laser 256] [--solver fft|multigrid] [--boxes 3]
                                        [--rounds 2] [--only full|patch] [--out FILE]

Prints one JSON line: slices/s of every timed box, the best and the median, and the resident envelope bytes of both.
--only runs one deck in this process (also for a run under rocprofv3 --kernel-trace: scripts/kstats.py reads its table)."""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def envelope_bytes(deck, decks):
    nxl, nyl, zlo, zhi = decks.laser_geometry(deck)[:4]
    levels = 3 if (deck["laser_solver"] >= 1 and deck["dt"] != 0.0) else 1
    return levels * 16 * nxl * nyl * (zhi - zlo + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--nz", type=int, default=2048)
    ap.add_argument("--n-laser", type=int, default=256)
    ap.add_argument("--solver", choices=["fft", "multigrid"], default="fft")
    ap.add_argument("--boxes", type=int, default=3, help="timed boxes per deck")
    ap.add_argument("--rounds", type=int, default=2, help="processes per deck")
    ap.add_argument("--only", choices=["full", "patch"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    if args.only is None:
        out = dict(n=args.n, nz=args.nz, n_laser=args.n_laser, solver=args.solver, boxes=args.boxes, rounds=args.rounds)
        for _ in range(args.rounds):
            for name in ("full", "patch"):
                cmd = [sys.executable, os.path.abspath(__file__), "--only", name, "--n", str(args.n), "--nz", str(args.nz), "--n-laser",
                       str(args.n_laser), "--solver", args.solver, "--boxes", str(args.boxes)]
                one = json.loads(subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True).stdout.strip().splitlines()[-1])[name]
                if name in out:
                    out[name]["slices_per_s"] += one["slices_per_s"]
                else:
                    out[name] = one
        for name in ("full", "patch"):
            r = sorted(out[name]["slices_per_s"])
            out[name].update(best=r[-1], median=r[len(r) // 2])
        line = json.dumps(out)
        print(line, flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return

    import torch
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    from hipace_amd import api, decks

    solver = 2 if args.solver == "multigrid" else 1
    all_decks = {"full": decks.config5(args.n, args.nz, solver), "patch": decks.config5_laser_patch(args.n, args.nz, args.n_laser, solver)}
    names = [args.only]
    engines = {}
    for name in names:
        engines[name] = api.SliceEngine(all_decks[name], tile_size=16, sort_period=128)
        engines[name].run_step()             # step 0, untimed
        engines[name].sync()
    rates = {name: [] for name in names}
    for _ in range(args.boxes):
        for name in names:
            e = engines[name]
            t0 = time.perf_counter()
            e.run_step()
            e.sync()
            rates[name].append(args.nz / (time.perf_counter() - t0))
    out = dict(n=args.n, nz=args.nz, n_laser=args.n_laser, solver=args.solver, boxes=args.boxes)
    for name in names:
        r = sorted(rates[name])
        out[name] = dict(slices_per_s=[round(v, 1) for v in rates[name]], best=round(r[-1], 1), median=round(r[len(r) // 2], 1),
                         laser_grid=engines[name].laser_grid(), envelope_bytes=envelope_bytes(all_decks[name], decks),
                         laser_vcycles=engines[name].laser_vcycles())
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
