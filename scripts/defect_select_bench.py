#!/usr/bin/env python3
"""Defect selection on the device-resident bench batch, timed against what it replaces.

Inputs: bench.py's default batch (256 x 128x128x24, synth_batch base_seed 0, 64 unique studies,
vary=True), vox [1.5, 1.5, 10].  Two steps, each a child process of its own under a time limit; the
second starts only when the first ended well:
  select      one profiled Batch.run (N4 on), then --rounds rounds of Batch.select_defect per source
              at medfilt 1: the defect_sel kernel class against the classify class of the same
              batch's runs, without and with the k-means label store, plus the host clock around
              select_defect + sync.  Counts at medfilt 0 are asserted equal to the run's n_lb12 /
              n_km0, and MEAN / medfilt 1 equal to the run's own maps.
  host-route  what a caller does without the selection: Batch.download() -> the map from the LB class
              volume with numpy -> Batch.upload_defect(), host clock.  Uses no call newer than
              upload_defect, so the same file times it on an older build (no such route exists for
              k-means there: the cuts never reach the host).
Prints one JSON line per step (profiles/defect_select.json holds them).
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
SOURCES = ("mean", "lb", "kmeans")


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
    return B


def step_select(args):
    B = bench_batch(args)
    opts = B.options(do_n4=True, vox=VOX, profile=True)
    B.run(opts)
    _, d0, bo0, lb0, res = B.download()
    for source, key in (("lb", "n_lb12"), ("kmeans", "n_km0")):   # parity at the timed size
        B.select_defect(source, 0)
        _, _, cnt = B.download_defect()
        assert list(cnt) == [getattr(r, key) for r in res], source
    B.select_defect("lb", 0)
    assert np.array_equal(B.download_defect()[0] != 0, np.isin(lb0, (1, 2)))
    B.select_defect("mean", 1)
    d, bo, _ = B.download_defect()
    assert np.array_equal(d, d0) and np.array_equal(bo, bo0)

    classify = []
    for _ in range(args.runs):
        B.reset_timers()
        B.run(opts)
        B.sync()
        ms, n, _ = B.kernel_time("classify")
        assert n == 1, n
        classify.append(ms)

    def rounds():
        kern = {s: [] for s in SOURCES}
        host = {s: [] for s in SOURCES}
        for s in SOURCES:   # warm-up
            B.select_defect(s, 1)
        B.sync()
        for _ in range(args.rounds):
            for s in SOURCES:
                B.reset_timers()
                t0 = time.perf_counter()
                B.select_defect(s, 1)
                B.sync()
                host[s].append(time.perf_counter() - t0)
                ms, n, _ = B.kernel_time("defect_sel")
                assert n == 1, n
                kern[s].append(ms)
        return ({s: stats(kern[s], 1e3, "us") for s in SOURCES},
                {s: stats(host[s], 1e3, "ms") for s in SOURCES})

    k0, h0 = rounds()
    B.download_defect(km=True)   # from here on the selection also stores the label map
    k1, h1 = rounds()
    B.close()
    cl = stats(classify, 1e3, "us")
    bound = 1.25 * cl["median_us"]
    out = {"what": "defect_select", "step": "select", "shape": list(args.shape), "batch": args.batch,
           "rounds": args.rounds, "classify_us": cl, "bound_us_1.25x_classify": round(bound, 3),
           "defect_sel_us": k0, "defect_sel_with_km_store_us": k1,
           "select_and_sync_host_ms": h0, "select_and_sync_with_km_store_host_ms": h1,
           "within_bound": {s: k0[s]["median_us"] <= bound for s in SOURCES},
           "within_bound_with_km_store": {s: k1[s]["median_us"] <= bound for s in SOURCES}}
    print(json.dumps(out))


def step_host_route(args):
    B = bench_batch(args)
    B.run(B.options(do_n4=True, vox=VOX))
    B.sync()

    def route():
        _, _, _, lb, _ = B.download()
        B.upload_defect(np.isin(lb, (1, 2)))

    route()
    ts = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        route()
        ts.append(time.perf_counter() - t0)
    parts = {"download": [], "numpy_map": [], "upload_defect": []}
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        _, _, _, lb, _ = B.download()
        t1 = time.perf_counter()
        m = np.isin(lb, (1, 2))
        t2 = time.perf_counter()
        B.upload_defect(m)
        t3 = time.perf_counter()
        for k, v in zip(parts, (t1 - t0, t2 - t1, t3 - t2)):
            parts[k].append(v)
    B.close()
    print(json.dumps({"what": "defect_select", "step": "host-route", "shape": list(args.shape),
                      "batch": args.batch, "rounds": args.rounds,
                      "lb_download_numpy_upload_host_ms": stats(ts, 1e3, "ms"),
                      "parts_host_ms": {k: stats(v, 1e3, "ms") for k, v in parts.items()},
                      "kmeans": "no host route: the cuts are not available on the host"}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--shape", type=int, nargs=3, default=(128, 128, 24))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5, help="profiled Batch.run calls for the classify class")
    ap.add_argument("--step", choices=("select", "host-route"), help="run this one step in this process")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per step")
    args = ap.parse_args()
    if args.rounds < 1 or args.runs < 1:
        sys.exit("--rounds and --runs must be >= 1")
    if args.step:
        {"select": step_select, "host-route": step_host_route}[args.step](args)
        return
    for step in ("select", "host-route"):   # chained: a failed or hung step ends the script
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--batch", str(args.batch),
               "--rounds", str(args.rounds), "--runs", str(args.runs), "--shape", *map(str, args.shape)]
        try:
            rc = subprocess.run(cmd, timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"step {step}: no end after {args.timeout} s; nothing further started")
        if rc != 0:
            sys.exit(f"step {step} ended with status {rc}; nothing further started")


if __name__ == "__main__":
    main()
