#!/usr/bin/env python3
"""The denoise option on the device-resident bench batch, timed against what it replaces.

Inputs: bench.py's default batch (256 x 128x128x24, synth_batch base_seed 0, 64 unique studies,
vary=True).  Two steps, each a child process of its own under a time limit; the second starts only when
the first ended well:
  device      Batch.noise_sigma once (its host time), then per (search, patch) setting --rounds rounds
              of upload-free Batch.denoise on the resident volumes, host clock from the enqueue to the
              stream's end, and the denoise_b kernel class of the same calls: voxel-offset pairs per
              second (voxels x (2 search + 1)^2 over the kernel time) and the kernel's share of the
              HBM roof on the 8 bytes per voxel it has to move (small: the kernel works in LDS).
  host-route  what a caller does without it: Batch.download_hp -> tests/denoise_ref.denoise per study
              -> Batch.upload, host clock, on --host-studies studies (the numpy filter takes seconds
              per study) and scaled to the batch by the study count; the result of those studies is
              asserted equal to the device's, bit for bit, outside the timed window.
Prints one JSON line per step (profiles/denoise.json holds them).
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
SETTINGS = ((3, 1), (5, 2))
STRENGTH = 2.0
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
    return B, hp, mk


def label(s):
    return "search%d_patch%d" % s


def step_device(args):
    B, hp, mk = bench_batch(args)
    B.run(B.options(do_n4=False, do_kmeans=False, vox=VOX, profile=True))   # (turns the kernel timers on)
    B.sync()
    t0 = time.perf_counter()
    sigma = B.noise_sigma()
    t_sigma = time.perf_counter() - t0
    assert np.isfinite(sigma).all() and (sigma > 0).all(), sigma
    voxels = float(np.prod(B.shape))
    out = {"what": "denoise", "step": "device", "shape": list(args.shape), "batch": args.batch,
           "rounds": args.rounds, "strength": STRENGTH, "noise_sigma_host_ms": round(t_sigma * 1e3, 3),
           "sigma_min_max": [float(sigma.min()), float(sigma.max())], "settings": {}}
    for s in SETTINGS:
        for _ in range(2):   # warm-up (the input of each round is the previous round's output: the
            B.denoise(sigma, STRENGTH, *s)   # kernel has no data-dependent work, so its time is the same)
        B.sync()
        host, kern, nbytes = [], [], 0.0
        for _ in range(args.rounds):
            B.reset_timers()
            t0 = time.perf_counter()
            B.denoise(sigma, STRENGTH, *s)
            B.sync()
            host.append(time.perf_counter() - t0)
            ms, n, nbytes = B.kernel_time("denoise_b")
            assert n == 1, n
            kern.append(ms)
        k = stats(kern, 1.0, "ms")
        sec = k["median_ms"] * 1e-3
        gbs = nbytes / sec / 1e9
        out["settings"][label(s)] = {
            "denoise_enqueue_to_done_host_ms": stats(host, 1e3, "ms"), "denoise_b_ms": k,
            "voxel_offset_pairs_per_s": round(voxels * (2 * s[0] + 1) ** 2 / sec, 1),
            "bytes_moved_per_launch": nbytes, "achieved_GBps": round(gbs, 1),
            "share_of_hbm_roof": round(gbs / HBM_PEAK_GBS, 4)}
    B.close()
    print(json.dumps(out))


def step_host_route(args):
    import denoise_ref as D
    B, hp, mk = bench_batch(args)
    sigma = B.noise_sigma()
    n = min(args.host_studies, args.batch)
    s = SETTINGS[0]
    ts = {"download_hp": [], "numpy": [], "upload": []}
    ref = None
    for _ in range(args.host_rounds):
        t0 = time.perf_counter()
        x = B.download_hp()
        t1 = time.perf_counter()
        ref = [D.denoise(x[q], sigma[q], STRENGTH, *s) for q in range(n)]
        t2 = time.perf_counter()
        B.upload(x, mk)
        t3 = time.perf_counter()
        ts["download_hp"].append(t1 - t0)
        ts["numpy"].append(t2 - t1)
        ts["upload"].append(t3 - t2)
    B.denoise(sigma, STRENGTH, *s)   # parity at the timed size
    got = B.download_hp()
    B.close()
    equal = all(np.array_equal(got[q].view(np.uint32), ref[q].view(np.uint32)) for q in range(n))
    assert equal
    per_study = float(np.median(ts["numpy"])) / n
    total = float(np.median(ts["download_hp"])) + per_study * args.batch + float(np.median(ts["upload"]))
    print(json.dumps({"what": "denoise", "step": "host-route", "shape": list(args.shape), "batch": args.batch,
                      "rounds": args.host_rounds, "setting": label(s), "studies_filtered_in_numpy": n,
                      "equal_to_the_device_result": equal,
                      "parts_host_ms": {k: stats(v, 1e3, "ms") for k, v in ts.items()},
                      "numpy_ms_per_study": round(per_study * 1e3, 3),
                      "download_numpy_upload_host_ms_scaled_to_the_batch": round(total * 1e3, 1)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--shape", type=int, nargs=3, default=(128, 128, 24))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--host-rounds", type=int, default=2, help="rounds of the host route")
    ap.add_argument("--host-studies", type=int, default=4, help="studies the host route filters in numpy")
    ap.add_argument("--step", choices=("device", "host-route"), help="run this one step in this process")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per step")
    args = ap.parse_args()
    if args.rounds < 1 or args.host_rounds < 1 or args.host_studies < 1:
        sys.exit("--rounds, --host-rounds and --host-studies must be >= 1")
    if args.step:
        {"device": step_device, "host-route": step_host_route}[args.step](args)
        return
    for step in ("device", "host-route"):   # chained: a failed or hung step ends the script
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--batch", str(args.batch),
               "--rounds", str(args.rounds), "--host-rounds", str(args.host_rounds),
               "--host-studies", str(args.host_studies), "--shape", *map(str, args.shape)]
        try:
            rc = subprocess.run(cmd, timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"step {step}: no end after {args.timeout} s; nothing further started")
        if rc != 0:
            sys.exit(f"step {step} ended with status {rc}; nothing further started")


if __name__ == "__main__":
    main()
