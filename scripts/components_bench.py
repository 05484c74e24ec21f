#!/usr/bin/env python3
"""The connected components of the device-resident bench batch, timed against what they replace.

Inputs: bench.py's default batch (256 x 128x128x24, synth_batch base_seed 0, 64 unique studies,
vary=True) after one plain run: its defect maps and its masks.  Two steps, each a child process of its
own under a time limit; the second starts only when the first ended well:
  device      --rounds rounds of Batch.components per connectivity on the run's defect maps, and with 6
              neighbours on the masks, on an all-ones map and on the checkerboard (the fewest and the
              most components): the comp_b kernel class with its algorithmic bytes (the source 1 read,
              the root 4 and the size 4 written per voxel) and their share of the 8 TB/s HBM spec; the
              host clock from the enqueue to the counts (download_components(root=False, size=False))
              and from the enqueue to the maps (8 bytes per voxel over the host link); the filter
              (Batch.filter_components, the labelling included) with min_size alone and with
              keep_largest = 2, the defect maps uploaded again before every round outside the clock.
  host-route  what a caller does without it: download_defect -> scipy.ndimage.label + np.bincount ->
              drop the components below min_size -> upload_defect, host clock, the labelling on
              --host-studies studies and scaled to the batch by the study count (an estimate); the
              result of those studies is asserted equal to the device's outside the timed window.
Prints one JSON line per step; with --out also writes both into that file (profiles/components.json).
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
EDGES = (2, 10, 100, 1000)
MIN_SIZE = 5
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


def kernel_rounds(B, rounds, source, conn, host_clock=False):
    for _ in range(2):   # warm-up
        B.components(source, conn, EDGES)
    B.sync()
    kern, counts, maps, nbytes, got = [], [], [], 0.0, None
    for _ in range(rounds):
        B.reset_timers()
        t0 = time.perf_counter()
        B.components(source, conn, EDGES)
        got = B.download_components(root=False, size=False)
        counts.append(time.perf_counter() - t0)
        ms, n, nbytes = B.kernel_time("comp_b")
        assert n == 1, n
        kern.append(ms)
    kk = stats(kern, 1e3, "us")
    gbs = nbytes / (kk["median_us"] * 1e-6) / 1e9
    out = {"comp_b_us": kk, "algorithmic_bytes_per_launch": nbytes, "achieved_GBps": round(gbs, 1),
           "share_of_hbm_spec": round(gbs / HBM_PEAK_GBS, 4),
           "n_set_total": int(got["stats"][:, 0].sum()), "n_components_total": int(got["stats"][:, 1].sum()),
           "largest_component": int(got["stats"][:, 2].max()),
           "class_components_total": got["counts"][:, :, 0].sum(axis=0).tolist()}
    if host_clock:
        for _ in range(max(2, rounds // 4)):
            t0 = time.perf_counter()
            B.components(source, conn, EDGES)
            full = B.download_components()
            maps.append(time.perf_counter() - t0)
        assert np.array_equal(full["counts"], got["counts"]) and np.array_equal(full["stats"], got["stats"])
        assert int((full["root"] >= 0).sum()) == out["n_set_total"]
        out["enqueue_to_counts_host_ms"] = stats(counts, 1e3, "ms")
        out["enqueue_to_maps_host_ms"] = stats(maps, 1e3, "ms")
    return out


def filter_rounds(B, rounds, defect, conn, min_size, keep_largest):
    """The filter on the defect maps, uploaded again before every round outside the clock: the comp_b
    class holds the labelling and the filter's passes (two timed spans), the border has its own."""
    kern, host, kept = [], [], None
    for i in range(rounds + 1):   # (the first is the warm-up)
        B.upload_defect(defect)
        B.reset_timers()
        t0 = time.perf_counter()
        kept = B.filter_components("defect", conn, min_size, keep_largest)
        t1 = time.perf_counter()
        ms, n, _ = B.kernel_time("comp_b")
        assert n == 2, n
        if i:
            kern.append(ms)
            host.append(t1 - t0)
    return {"comp_b_us": stats(kern, 1e3, "us"), "enqueue_to_kept_host_ms": stats(host, 1e3, "ms"),
            "components_kept_total": int(kept[:, 0].sum()), "voxels_kept_total": int(kept[:, 1].sum())}


def step_device(args):
    B, hp, mk = bench_batch(args)
    defect = B.download_defect()[0].copy()
    out = {"what": "components", "step": "device", "shape": list(args.shape), "batch": args.batch,
           "rounds": args.rounds, "edges": list(EDGES), "defect_fraction": round(float((defect != 0).mean()), 4),
           "masked_fraction": round(float((mk != 0).mean()), 4)}
    out["bench_defect_maps"] = {"conn%d" % c: kernel_rounds(B, args.rounds, "defect", c, c == 6) for c in (4, 8, 6, 26)}
    out["bench_masks_conn6"] = kernel_rounds(B, args.rounds, "mask", 6)
    out["filter_min_size_%d_conn6" % MIN_SIZE] = filter_rounds(B, args.rounds, defect, 6, MIN_SIZE, 0)
    out["filter_keep_largest_2_conn6"] = filter_rounds(B, args.rounds, defect, 6, 1, 2)
    B.upload_defect(np.ones_like(defect))
    out["all_ones"] = {"conn%d" % c: kernel_rounds(B, args.rounds, "defect", c) for c in (6, 26)}
    rr, cc = np.mgrid[0:args.shape[0], 0:args.shape[1]]
    B.upload_defect(np.broadcast_to((((rr + cc) % 2) == 0)[None, :, :, None], defect.shape))
    out["checkerboard"] = {"conn%d" % c: kernel_rounds(B, args.rounds, "defect", c) for c in (4, 26)}
    B.close()
    print(json.dumps(out))


def host_label(defect, conn=6):
    """One study on the host: scipy's labels and their sizes."""
    from scipy import ndimage as ndi
    lab, n = ndi.label(defect != 0, ndi.generate_binary_structure(3, 1 if conn == 6 else 3))
    return lab, np.bincount(lab.ravel(), minlength=n + 1)


def step_host_route(args):
    B, hp, mk = bench_batch(args)
    n = min(args.host_studies, args.batch)
    ts = {"download_defect": [], "scipy_label_bincount_filter": [], "upload_defect": []}
    d = filt = sizes = None
    for _ in range(args.host_rounds):
        t0 = time.perf_counter()
        d = B.download_defect()[0]
        t1 = time.perf_counter()
        filt, sizes = d.copy(), []
        for q in range(n):
            lab, sz = host_label(d[q])
            sz[0] = 0
            filt[q] = np.where(sz[lab] >= MIN_SIZE, d[q], 0)
            sizes.append(sz[lab])
        t2 = time.perf_counter()
        B.upload_defect(d)   # (the unfiltered maps again: the transfer is what is timed)
        t3 = time.perf_counter()
        ts["download_defect"].append(t1 - t0)
        ts["scipy_label_bincount_filter"].append(t2 - t1)
        ts["upload_defect"].append(t3 - t2)
    B.components("defect", 6)   # parity at the timed size
    got = B.download_components()
    equal = all(np.array_equal(got["size"][q], sizes[q]) for q in range(n))
    kept = B.filter_components("defect", 6, MIN_SIZE, 0)
    after = B.download_defect()[0]
    equal = equal and all(np.array_equal(after[q], filt[q]) and kept[q, 1] == np.count_nonzero(filt[q]) for q in range(n))
    assert equal
    per_study = float(np.median(ts["scipy_label_bincount_filter"])) / n
    total = float(np.median(ts["download_defect"])) + float(np.median(ts["upload_defect"])) + per_study * args.batch
    out = {"what": "components", "step": "host-route", "shape": list(args.shape), "batch": args.batch,
           "rounds": args.host_rounds, "studies_on_the_host": n, "equal_to_the_device_result": equal,
           "min_size": MIN_SIZE, "parts_host_ms": {q: stats(v, 1e3, "ms") for q, v in ts.items()},
           "scipy_and_numpy_ms_per_study": round(per_study * 1e3, 3),
           "download_scipy_upload_host_ms_scaled_to_the_batch": round(total * 1e3, 1)}
    B.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--shape", type=int, nargs=3, default=(128, 128, 24))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--host-rounds", type=int, default=2, help="rounds of the host route")
    ap.add_argument("--host-studies", type=int, default=4, help="studies the host route labels")
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
            json.dump({"what": "components", "script": "scripts/components_bench.py", "device": "one MI355X",
                       "this_change": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
