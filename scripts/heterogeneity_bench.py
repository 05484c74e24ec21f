#!/usr/bin/env python3
"""The local ventilation heterogeneity on the device-resident bench batch, timed against what it
replaces.

Inputs: bench.py's default batch (256 x 128x128x24, synth_batch base_seed 0, 64 unique studies,
vary=True) after one plain run.  Two steps, each a child process of its own under a time limit; the
second starts only when the first ended well:
  device      per radius (1 and 5, min_count the default majority, 100 bins of [0, 1)) --rounds rounds
              of Batch.heterogeneity on the resident volumes: the het_b kernel class with the bytes it
              has to move (x 4, mask 1, the map 4 per voxel) and their share of the 8 TB/s HBM spec;
              the host clock from the enqueue to the counts (download_heterogeneity(map=False)) and
              from the enqueue to the map (map=True, 4 bytes per voxel over the host link).
  host-route  what a caller does without it: Batch.download(n4=True) -> tests/heterogeneity_ref per
              study, host clock, on --host-studies studies and scaled to the batch by the study count;
              the result of those studies is asserted equal to the device's, bit for bit, outside the
              timed window.
Prints one JSON line per step; with --out also writes both into that file (profiles/heterogeneity.json).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

VOX = (1.5, 1.5, 10.0)
RADII = (1, 5)
BINS, HI = 100, 1.0
HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec, as bench.py


def stats(ts, scale, unit):
    ts = np.asarray(ts) * scale
    return {"median_" + unit: round(float(np.median(ts)), 3), "min_" + unit: round(float(ts.min()), 3),
            "max_" + unit: round(float(ts.max()), 3), "n": int(ts.size)}


def bench_batch(args):
    from vent_analysis_amd import _lib
    from vent_analysis_amd.synth import synth_batch
    R, C, Z = args.shape
    hp, mk = synth_batch(R, C, Z, args.batch, base_seed=0, unique=64, vary=True)
    B = _lib.Batch(R, C, Z, args.batch)
    B.upload(hp, mk)
    B.run(B.options(do_n4=False, do_kmeans=False, vox=VOX, profile=True))   # (turns the kernel timers on)
    B.sync()
    return B, hp, mk


def step_device(args):
    B, hp, mk = bench_batch(args)
    out = {"what": "heterogeneity", "step": "device", "shape": list(args.shape), "batch": args.batch,
           "rounds": args.rounds, "bins": BINS, "hi": HI, "masked_fraction": round(float((mk != 0).mean()), 4),
           "radii": {}}
    for k in RADII:
        for _ in range(2):   # warm-up
            B.heterogeneity(k, None, BINS, HI)
        B.sync()
        kern, counts, maps, nbytes = [], [], [], 0.0
        for _ in range(args.rounds):
            B.reset_timers()
            t0 = time.perf_counter()
            B.heterogeneity(k, None, BINS, HI)
            got = B.download_heterogeneity(map=False)
            counts.append(time.perf_counter() - t0)
            ms, n, nbytes = B.kernel_time("het_b")
            assert n == 1, n
            kern.append(ms)
        for _ in range(max(2, args.rounds // 4)):
            t0 = time.perf_counter()
            B.heterogeneity(k, None, BINS, HI)
            full = B.download_heterogeneity(map=True)
            maps.append(time.perf_counter() - t0)
        assert np.array_equal(full["stats"], got["stats"]) and got["stats"][:, 0].any()
        kk = stats(kern, 1e3, "us")
        gbs = nbytes / (kk["median_us"] * 1e-6) / 1e9
        out["radii"]["radius%d" % k] = {
            "het_b_us": kk, "bytes_moved_per_launch": nbytes, "achieved_GBps": round(gbs, 1),
            "share_of_hbm_spec": round(gbs / HBM_PEAK_GBS, 4),
            "enqueue_to_counts_host_ms": stats(counts, 1e3, "ms"),
            "enqueue_to_map_host_ms": stats(maps, 1e3, "ms"),
            "index_min_max": [float(np.nanmin(got["index"])), float(np.nanmax(got["index"]))]}
    B.close()
    print(json.dumps(out))


def step_host_route(args):
    import heterogeneity_ref as H
    B, hp, mk = bench_batch(args)
    n = min(args.host_studies, args.batch)
    out = {"what": "heterogeneity", "step": "host-route", "shape": list(args.shape), "batch": args.batch,
           "rounds": args.host_rounds, "studies_in_numpy": n, "radii": {}}
    for k in RADII:
        mc = (2 * k + 1) ** 2 // 2 + 1
        ts = {"download_n4": [], "numpy": []}
        ref = None
        for _ in range(args.host_rounds):
            t0 = time.perf_counter()
            x = B.download(n4=True, maps=False)[0]
            t1 = time.perf_counter()
            ref = H.reference(x[:n], mk[:n] != 0, k, mc, BINS, HI)
            t2 = time.perf_counter()
            ts["download_n4"].append(t1 - t0)
            ts["numpy"].append(t2 - t1)
        B.heterogeneity(k, None, BINS, HI)   # parity at the timed size
        got = B.download_heterogeneity()
        equal = bool(np.array_equal(got["map"][:n].view(np.uint32), ref[0].view(np.uint32))
                     and np.array_equal(got["hist"][:n], ref[1]) and np.array_equal(got["stats"][:n], ref[2]))
        assert equal
        per_study = float(np.median(ts["numpy"])) / n
        total = float(np.median(ts["download_n4"])) + per_study * args.batch
        out["radii"]["radius%d" % k] = {
            "equal_to_the_device_result": equal,
            "parts_host_ms": {q: stats(v, 1e3, "ms") for q, v in ts.items()},
            "numpy_ms_per_study": round(per_study * 1e3, 3),
            "download_and_numpy_host_ms_scaled_to_the_batch": round(total * 1e3, 1)}
    B.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--shape", type=int, nargs=3, default=(128, 128, 24))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--host-rounds", type=int, default=2, help="rounds of the host route")
    ap.add_argument("--host-studies", type=int, default=4, help="studies the host route computes in numpy")
    ap.add_argument("--step", choices=("device", "host-route"), help="run this one step in this process")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per step")
    ap.add_argument("--out", help="also write both steps' results into this JSON file")
    args = ap.parse_args()
    if args.rounds < 1 or args.host_rounds < 1 or args.host_studies < 1:
        sys.exit("--rounds, --host-rounds and --host-studies must be >= 1")
    if args.step:
        {"device": step_device, "host-route": step_host_route}[args.step](args)
        return
    results = {}
    for step in ("device", "host-route"):   # chained: a failed or hung step ends the script
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--batch", str(args.batch),
               "--rounds", str(args.rounds), "--host-rounds", str(args.host_rounds),
               "--host-studies", str(args.host_studies), "--shape", *map(str, args.shape)]
        try:
            p = subprocess.run(cmd, timeout=args.timeout, stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            sys.exit(f"step {step}: no end after {args.timeout} s; nothing further started")
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            sys.exit(f"step {step} ended with status {p.returncode}; nothing further started")
        results[step.replace("-", "_")] = json.loads(p.stdout.strip().splitlines()[-1])
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"what": "heterogeneity", "script": "scripts/heterogeneity_bench.py", "device": "one MI355X",
                       "this_change": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
