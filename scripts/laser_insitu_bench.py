#!/usr/bin/env python3
"""Cost of the in-situ laser reductions (hps_engine_set_insitu_laser) per slice on BASELINE config 5 with the envelope
on a centred patch (decks.config5_laser_patch): the same deck with the switch off and on, whole boxes through
SliceEngine.run_step, a host clock around each box that ends in a device synchronise, the first box untimed.  One process per
setting, the two alternating --rounds times (as scripts/laser_patch_bench.py).

    python scripts/laser_insitu_bench.py [--n 1024] [--nz 2048] [--n-laser 256] [--boxes 3] [--rounds 3] [--only off|on] [--child-timeout S] [--out FILE]

Prints one JSON line: slices/s of every timed box of both settings, the best and the median.  --only runs one setting in this
process (also for a run under rocprofv3 --kernel-trace: scripts/kstats.py reads its table)."""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--nz", type=int, default=2048)
    ap.add_argument("--n-laser", type=int, default=256)
    ap.add_argument("--boxes", type=int, default=3, help="timed boxes per process")
    ap.add_argument("--rounds", type=int, default=3, help="processes per setting")
    ap.add_argument("--child-timeout", type=float, default=300.0, help="seconds one child process may take")
    ap.add_argument("--only", choices=["off", "on"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    if args.only is None:
        out = dict(n=args.n, nz=args.nz, n_laser=args.n_laser, boxes=args.boxes, rounds=args.rounds, off=[], on=[])
        for _ in range(args.rounds):
            for name in ("off", "on"):
                cmd = [sys.executable, os.path.abspath(__file__), "--only", name, "--n", str(args.n), "--nz", str(args.nz), "--n-laser",
                       str(args.n_laser), "--boxes", str(args.boxes)]
                # a child that hangs ends the measurement (TimeoutExpired) instead of holding the device
                done = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True, timeout=args.child_timeout)
                one = json.loads(done.stdout.strip().splitlines()[-1])
                out[name] += one["slices_per_s"]
        for name in ("off", "on"):
            r = sorted(out[name])
            out[name + "_best"], out[name + "_median"] = r[-1], r[len(r) // 2]
        line = json.dumps(out)
        print(line, flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return

    import torch
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    from hipace_amd import api, decks

    e = api.SliceEngine(decks.config5_laser_patch(args.n, args.nz, args.n_laser, 1), tile_size=16, sort_period=128)
    if args.only == "on":
        e.set_insitu_laser()
    e.run_step()             # step 0, untimed
    e.sync()
    rates = []
    for _ in range(args.boxes):
        t0 = time.perf_counter()
        e.run_step()
        e.sync()
        rates.append(round(args.nz / (time.perf_counter() - t0), 1))
    out = dict(setting=args.only, slices_per_s=rates)
    if args.only == "on":
        out["max_a2"] = float(e.insitu_laser()["sum"]["max(|a|^2)"])
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
