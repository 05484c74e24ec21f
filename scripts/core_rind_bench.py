#!/usr/bin/env python3
"""The core-rind analysis on the device-resident bench batch, timed against what it replaces.

Inputs: bench.py's default batch (256 x 128x128x24, synth_batch base_seed 0, 64 unique studies,
vary=True) after one plain run.  Two steps, each a child process of its own under a time limit; the
second starts only when the first ended well:
  device      --rounds rounds of Batch.core_rind (edges 1.5 and 3.5 pixels, with the defect column) on
              the resident masks, and again on an all-ones mask, the deepest search: the depth_b kernel
              class with its algorithmic bytes (mask 1 and defect 1 read, the map 2 written per voxel)
              and their share of the 8 TB/s HBM spec; the host clock from the enqueue to the counts
              (download_core_rind(map=False)) and from the enqueue to the map (2 bytes per voxel over
              the host link).
  host-route  what a caller does without it: download_mask + download_defect ->
              scipy.ndimage.distance_transform_edt on every 1-padded slice -> numpy band counts, host
              clock, on --host-studies studies and scaled to the batch by the study count (an estimate);
              the result of those studies is asserted equal to the device's outside the timed window.
Prints one JSON line per step; with --out also writes both into that file (profiles/core_rind.json).
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

VOX = (1.5, 1.5, 10.0)
EDGES = (1.5, 3.5)
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


def kernel_rounds(B, rounds, host_clock):
    for _ in range(2):   # warm-up
        B.core_rind(EDGES)
    B.sync()
    kern, counts, maps, nbytes, got = [], [], [], 0.0, None
    for _ in range(rounds):
        B.reset_timers()
        t0 = time.perf_counter()
        B.core_rind(EDGES)
        got = B.download_core_rind(map=False)
        counts.append(time.perf_counter() - t0)
        ms, n, nbytes = B.kernel_time("depth_b")
        assert n == 1, n
        kern.append(ms)
    kk = stats(kern, 1e3, "us")
    gbs = nbytes / (kk["median_us"] * 1e-6) / 1e9
    out = {"depth_b_us": kk, "algorithmic_bytes_per_launch": nbytes, "achieved_GBps": round(gbs, 1),
           "share_of_hbm_spec": round(gbs / HBM_PEAK_GBS, 4),
           "n_mask_total": int(got["stats"][:, 0].sum()), "max_depth_px": round(float(np.sqrt(got["stats"][:, 1].max())), 2),
           "band_voxels_total": got["counts"][:, :, 0].sum(axis=0).tolist()}
    if host_clock:
        for _ in range(max(2, rounds // 4)):
            t0 = time.perf_counter()
            B.core_rind(EDGES)
            full = B.download_core_rind(map=True)
            maps.append(time.perf_counter() - t0)
        assert np.array_equal(full["counts"], got["counts"]) and got["counts"][:, :, 1].any()
        out["enqueue_to_counts_host_ms"] = stats(counts, 1e3, "ms")
        out["enqueue_to_map_host_ms"] = stats(maps, 1e3, "ms")
    return out


def step_device(args):
    B, hp, mk = bench_batch(args)
    out = {"what": "core_rind", "step": "device", "shape": list(args.shape), "batch": args.batch,
           "rounds": args.rounds, "edges_px": list(EDGES), "masked_fraction": round(float((mk != 0).mean()), 4)}
    out["bench_masks"] = kernel_rounds(B, args.rounds, True)
    B.upload(None, np.ones_like(mk))   # the deepest search; the run's defect maps stay resident
    out["all_ones_mask"] = kernel_rounds(B, args.rounds, False)
    B.close()
    print(json.dumps(out))


def host_route(mask, defect, thr):
    """One study on the host: scipy's exact EDT of every 1-padded slice, squared, and the band counts."""
    from scipy import ndimage as ndi
    M = mask != 0
    d2 = np.empty(M.shape, np.int64)
    for z in range(M.shape[2]):
        e = ndi.distance_transform_edt(np.pad(M[:, :, z], 1))[1:-1, 1:-1]
        d2[:, :, z] = np.rint(e * e)
    band = np.searchsorted(thr, np.minimum(d2, 65535)[M], side="right")
    counts = np.zeros((len(thr) + 1, 2), np.int64)
    counts[:, 0] = np.bincount(band, minlength=len(thr) + 1)
    counts[:, 1] = np.bincount(band[(defect != 0)[M]], minlength=len(thr) + 1)
    return np.minimum(d2, 65535).astype(np.uint16), counts, np.array([M.sum(), d2.max()], np.int64)


def step_host_route(args):
    from vent_analysis_amd import _lib
    B, hp, mk = bench_batch(args)
    n = min(args.host_studies, args.batch)
    thr = _lib.depth_thresholds(EDGES).astype(np.int64)
    ts = {"download_mask": [], "download_defect": [], "scipy_and_numpy": []}
    ref = None
    for _ in range(args.host_rounds):
        t0 = time.perf_counter()
        m = B.download_mask()
        t1 = time.perf_counter()
        d = B.download_defect()[0]
        t2 = time.perf_counter()
        ref = [host_route(m[q], d[q], thr) for q in range(n)]
        t3 = time.perf_counter()
        ts["download_mask"].append(t1 - t0)
        ts["download_defect"].append(t2 - t1)
        ts["scipy_and_numpy"].append(t3 - t2)
    B.core_rind(EDGES)   # parity at the timed size
    got = B.download_core_rind()
    equal = all(np.array_equal(got["d2"][q], ref[q][0]) and np.array_equal(got["counts"][q], ref[q][1])
                and np.array_equal(got["stats"][q], ref[q][2]) for q in range(n))
    assert equal
    per_study = float(np.median(ts["scipy_and_numpy"])) / n
    total = float(np.median(ts["download_mask"])) + float(np.median(ts["download_defect"])) + per_study * args.batch
    out = {"what": "core_rind", "step": "host-route", "shape": list(args.shape), "batch": args.batch,
           "rounds": args.host_rounds, "studies_on_the_host": n, "equal_to_the_device_result": equal,
           "parts_host_ms": {q: stats(v, 1e3, "ms") for q, v in ts.items()},
           "scipy_and_numpy_ms_per_study": round(per_study * 1e3, 3),
           "downloads_scipy_and_numpy_host_ms_scaled_to_the_batch": round(total * 1e3, 1)}
    B.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--shape", type=int, nargs=3, default=(128, 128, 24))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--host-rounds", type=int, default=2, help="rounds of the host route")
    ap.add_argument("--host-studies", type=int, default=4, help="studies the host route computes")
    ap.add_argument("--step", choices=("device", "host-route"), help="run this one step in this process")
    ap.add_argument("--timeout", type=int, default=180, help="seconds per step")
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
            json.dump({"what": "core_rind", "script": "scripts/core_rind_bench.py", "device": "one MI355X",
                       "this_change": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
