#!/usr/bin/env python3
"""The ventilation distribution of the device-resident bench batch, timed against what it replaces.

Inputs: bench.py's default batch (256 x 128x128x24, synth_batch base_seed 0, 64 unique studies,
vary=True), vox [1.5, 1.5, 10].  Two steps, each a child process of its own under a time limit; the
second starts only when the first ended well:
  device      one profiled Batch.run (N4 on), then --rounds rounds per (norm, bins, hi) setting of
              Batch.distribution + download_distribution, host clock from the enqueue to the counts
              on the host, and the dist_b kernel class of the same calls with its share of the HBM
              roof on the 7 bytes per voxel it reads.
  host-route  what a caller does without it: Batch.download(n4=True) -> the numpy form of the same
              semantics (float32 division and multiply, np.bincount, sums over the slice axes),
              host clock.  Uses no call newer than download, so the same file times it on an older
              build; on a build that has Batch.distribution the two results are asserted equal at
              the timed size, outside the timed window.
Prints one JSON line per step (profiles/distribution.json holds them).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

VOX = (1.5, 1.5, 10.0)
SETTINGS = (("p99", 1024, 1.5), ("p99", 100, 1.5), ("mean", 100, 2.0))
HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec, as bench.py
F32 = np.float32


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
    return B, np.ascontiguousarray(mk, dtype=np.uint8)


def label(s):
    return "%s_%d_%g" % s


def step_device(args):
    B, _ = bench_batch(args)
    B.run(B.options(do_n4=True, vox=VOX, profile=True))
    res = B.download(maps=False)[4]
    B.distribution()
    got = B.download_distribution()
    sl = got["slice_counts"]
    assert list(sl[:, :, 0].sum(axis=1)) == [r.n_mask for r in res]       # parity at the timed size
    assert list(sl[:, :, 1].sum(axis=1)) == [r.n_defect for r in res]
    assert list(sl[:, :, 2:4].sum(axis=(1, 2))) == [r.n_lb12 for r in res]
    assert list(got["hist"].sum(axis=1, dtype=np.int64) + got["outside"].sum(axis=1)) == [r.n_mask for r in res]
    out = {"what": "distribution", "step": "device", "shape": list(args.shape), "batch": args.batch,
           "rounds": args.rounds, "settings": {}}
    for s in SETTINGS:
        for _ in range(3):   # warm-up
            B.distribution(*s)
            B.download_distribution()
        host, kern, nbytes = [], [], 0.0
        for _ in range(args.rounds):
            B.reset_timers()
            t0 = time.perf_counter()
            B.distribution(*s)
            B.download_distribution()
            host.append(time.perf_counter() - t0)
            ms, n, nbytes = B.kernel_time("dist_b")
            assert n == 1, n
            kern.append(ms)
        k = stats(kern, 1e3, "us")
        gbs = nbytes / (k["median_us"] * 1e-6) / 1e9
        out["settings"][label(s)] = {
            "distribution_and_download_host_ms": stats(host, 1e3, "ms"), "dist_b_us": k,
            "bytes_read_per_launch": nbytes, "achieved_GBps": round(gbs, 1),
            "share_of_hbm_roof": round(gbs / HBM_PEAK_GBS, 4)}
    B.close()
    print(json.dumps(out))


def numpy_distribution(n4, mk, d, lb, res, norm, bins, hi):
    """The numpy form of vh_batch_distribution's semantics over a downloaded batch."""
    nb, _, _, Z = n4.shape
    hist = np.zeros((nb, bins), np.uint32)
    outside = np.zeros((nb, 2), np.int64)
    sl = np.zeros((nb, Z, 8), np.int64)
    scale = F32(F32(bins) / F32(hi))
    sl[:, :, 0] = (mk != 0).sum(axis=(1, 2))
    sl[:, :, 1] = (d != 0).sum(axis=(1, 2))
    for c in range(1, 7):
        sl[:, :, c + 1] = (lb == c).sum(axis=(1, 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        for q in range(nb):
            dv = F32(res[q].mean_anchor if norm == "mean" else res[q].p99)
            nv = n4[q][mk[q] != 0] / dv
            inside = (nv >= 0) & (nv < F32(hi))
            bi = np.minimum(bins - 1, (nv[inside] * scale).astype(np.int64))
            hist[q] = np.bincount(bi, minlength=bins)
            below = int((nv < 0).sum())
            outside[q] = (below, nv.size - int(inside.sum()) - below)
    return dict(hist=hist, outside=outside, slice_counts=sl)


def step_host_route(args):
    B, mk = bench_batch(args)
    B.run(B.options(do_n4=True, vox=VOX))
    B.sync()
    s = SETTINGS[0]

    def route():
        n4, d, _, lb, res = B.download(n4=True)
        return numpy_distribution(n4, mk, d, lb, res, *s)

    ref = route()
    if hasattr(B, "distribution"):   # parity at the timed size
        B.distribution(*s)
        got = B.download_distribution()
        assert all(np.array_equal(got[k], ref[k]) for k in ref)
    ts = []
    parts = {"download_n4_and_maps": [], "numpy": []}
    for _ in range(args.host_rounds):
        t0 = time.perf_counter()
        n4, d, _, lb, res = B.download(n4=True)
        t1 = time.perf_counter()
        numpy_distribution(n4, mk, d, lb, res, *s)
        t2 = time.perf_counter()
        ts.append(t2 - t0)
        parts["download_n4_and_maps"].append(t1 - t0)
        parts["numpy"].append(t2 - t1)
    B.close()
    print(json.dumps({"what": "distribution", "step": "host-route", "shape": list(args.shape),
                      "batch": args.batch, "rounds": args.host_rounds, "setting": label(s),
                      "equal_to_the_device_result": hasattr(B, "distribution"),
                      "download_numpy_host_ms": stats(ts, 1e3, "ms"),
                      "parts_host_ms": {k: stats(v, 1e3, "ms") for k, v in parts.items()}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--shape", type=int, nargs=3, default=(128, 128, 24))
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--host-rounds", type=int, default=5, help="rounds of the host route (seconds each)")
    ap.add_argument("--step", choices=("device", "host-route"), help="run this one step in this process")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per step")
    args = ap.parse_args()
    if args.rounds < 1 or args.host_rounds < 1:
        sys.exit("--rounds and --host-rounds must be >= 1")
    if args.step:
        {"device": step_device, "host-route": step_host_route}[args.step](args)
        return
    for step in ("device", "host-route"):   # chained: a failed or hung step ends the script
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--batch", str(args.batch),
               "--rounds", str(args.rounds), "--host-rounds", str(args.host_rounds),
               "--shape", *map(str, args.shape)]
        try:
            rc = subprocess.run(cmd, timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"step {step}: no end after {args.timeout} s; nothing further started")
        if rc != 0:
            sys.exit(f"step {step} ended with status {rc}; nothing further started")


if __name__ == "__main__":
    main()
