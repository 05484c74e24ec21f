#!/usr/bin/env python3
"""The regional analysis of the device-resident bench batch, timed against its yardstick and against
what it replaces.

Inputs: bench.py's default batch (256 x 128x128x24, synth_batch base_seed 0, 64 unique studies,
vary=True), vox [1.5, 1.5, 10].  Two steps, each a child process of its own under a time limit; the
second starts only when the first ended well:
  device      one profiled Batch.run (N4 on), then --rounds rounds of each configuration -- (3, 1, 1)
              lateral, (3, 1, 2) lateral, a 5-zone label volume -- and of Batch.distribution at
              (mean, 100, 1.5), the four alternating inside every round: the zones_b kernel class
              (profile, tables, map and count kernels between one pair of events) against the bytes
              they have to move, dist_b in the same session as the yardstick (the count sweep moves
              its 7 B/voxel plus the zone byte), and the host clock from the enqueue to the counts on
              the host and to the counts and the map on the host.
  host-route  what a caller does without it: download(n4=True) + download_mask + the numpy reference
              (tests/zones_ref.py) on --host-studies studies, scaled to the batch: an estimate, marked
              as one.  The device result is asserted equal on those studies, outside the timed window.
Prints one JSON line per step (profiles/zones.json holds them).
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
DIST = ("mean", 100, 1.5)
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
    return B


def configurations(B):
    """name -> Batch.zones keywords; the label volume is the (5, 1, 1) by-count map of the batch itself."""
    B.zones((5, 1, 1), False, "count")
    labels = np.array(B.download_zones()["map"])
    return {"3x1x1_lateral": dict(parts=(3, 1, 1), lateral=True),
            "3x1x2_lateral": dict(parts=(3, 1, 2), lateral=True),
            "labels_5": dict(labels=labels, n_zones=5)}


def step_device(args):
    B = bench_batch(args)
    B.run(B.options(do_n4=True, vox=VOX, profile=True))
    res = B.download(maps=False)[4]
    cfg = configurations(B)
    B.distribution(*DIST)
    dist = B.download_distribution()
    for kw in cfg.values():   # parity at the timed size
        B.zones(**kw)
        got = B.download_zones(map=False)
        assert list(got["counts"][:, :, 0].sum(axis=1)) == [r.n_mask for r in res]
        assert list(got["counts"][:, :, 2:4].sum(axis=(1, 2))) == [r.n_lb12 for r in res]
        assert np.array_equal(got["hist"].sum(axis=1, dtype=np.uint32), dist["hist"])
        assert np.array_equal(got["stats"][:, :, 1:3].sum(axis=1), dist["outside"])
    for _ in range(3):   # warm-up
        for kw in cfg.values():
            B.zones(**kw)
            B.download_zones()
        B.distribution(*DIST)
        B.download_distribution()
    kern = {k: [] for k in cfg}
    counts_ms = {k: [] for k in cfg}
    map_ms = {k: [] for k in cfg}
    nbytes = {}
    dist_us, dist_ms, dist_bytes = [], [], 0.0
    for _ in range(args.rounds):
        for name, kw in cfg.items():
            B.reset_timers()
            t0 = time.perf_counter()
            B.zones(**kw)
            B.download_zones(map=False)
            counts_ms[name].append(time.perf_counter() - t0)
            ms, n, nbytes[name] = B.kernel_time("zones_b")
            assert n == 1, n
            kern[name].append(ms)
            t0 = time.perf_counter()
            B.zones(**kw)
            B.download_zones()
            map_ms[name].append(time.perf_counter() - t0)
        B.reset_timers()
        t0 = time.perf_counter()
        B.distribution(*DIST)
        B.download_distribution()
        dist_ms.append(time.perf_counter() - t0)
        ms, n, dist_bytes = B.kernel_time("dist_b")
        assert n == 1, n
        dist_us.append(ms)
    B.close()
    out = {"what": "zones", "step": "device", "shape": list(args.shape), "batch": args.batch, "rounds": args.rounds,
           "configurations": {}}
    d = stats(dist_us, 1e3, "us")
    out["dist_b_yardstick"] = {"setting": "%s_%d_%g" % DIST, "dist_b_us": d, "bytes_read_per_launch": dist_bytes,
                               "achieved_GBps": round(dist_bytes / (d["median_us"] * 1e-6) / 1e9, 1),
                               "distribution_and_download_host_ms": stats(dist_ms, 1e3, "ms")}
    for name in cfg:
        k = stats(kern[name], 1e3, "us")
        gbs = nbytes[name] / (k["median_us"] * 1e-6) / 1e9
        out["configurations"][name] = {
            "zones_b_us": k, "bytes_moved_per_call": nbytes[name], "achieved_GBps": round(gbs, 1),
            "share_of_hbm_roof": round(gbs / HBM_PEAK_GBS, 4),
            "zones_b_over_dist_b": round(k["median_us"] / d["median_us"], 3),
            "enqueue_to_counts_on_host_ms": stats(counts_ms[name], 1e3, "ms"),
            "enqueue_to_counts_and_map_on_host_ms": stats(map_ms[name], 1e3, "ms")}
    print(json.dumps(out))


def step_host_route(args):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
    import zones_ref as ZR
    B = bench_batch(args)
    B.run(B.options(do_n4=True, vox=VOX))
    B.sync()
    n = min(args.host_studies, args.batch)
    kw = dict(parts=(3, 1, 2), lateral=True, by=ZR.EXTENT, norm="mean", bins=100, hi=1.5)

    def numpy_part(n4, mk, d, lb):
        return [ZR.reference(n4[q], mk[q], d[q], lb[q], **kw) for q in range(n)]

    B.zones((3, 1, 2), True)
    got = B.download_zones()
    down, ref_s = [], []
    for _ in range(args.host_rounds):
        t0 = time.perf_counter()
        n4, d, _, lb, _ = B.download(n4=True)
        mk = B.download_mask()
        t1 = time.perf_counter()
        refs = numpy_part(n4, mk, d, lb)
        t2 = time.perf_counter()
        down.append(t1 - t0)
        ref_s.append(t2 - t1)
    ZR.assert_equal({k: got[k][:n] for k in ("map", "counts", "hist", "stats", "geom")}, refs)
    B.close()
    scaled = [a + b * args.batch / n for a, b in zip(down, ref_s)]
    print(json.dumps({"what": "zones", "step": "host-route", "shape": list(args.shape), "batch": args.batch,
                      "rounds": args.host_rounds, "setting": "3x1x2_lateral_mean_100_1.5",
                      "equal_to_the_device_result_on_the_studies_computed": True, "studies_computed": n,
                      "download_n4_maps_mask_host_ms": stats(down, 1e3, "ms"),
                      "numpy_reference_of_the_studies_computed_host_ms": stats(ref_s, 1e3, "ms"),
                      "estimate_download_plus_numpy_whole_batch_host_ms": stats(scaled, 1e3, "ms"),
                      "note": "an estimate: the numpy time of the studies computed, scaled by batch / studies"}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--shape", type=int, nargs=3, default=(128, 128, 24))
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--host-rounds", type=int, default=3)
    ap.add_argument("--host-studies", type=int, default=4, help="studies the numpy route computes (it is scaled)")
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
