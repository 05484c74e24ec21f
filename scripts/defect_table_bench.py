#!/usr/bin/env python3
"""The defect table of the device-resident bench batch, timed against what it replaces.

Inputs: bench.py's default batch (256 x 128x128x24, synth_batch base_seed 0, 64 unique studies,
vary=True) after one plain run: its defect maps and its masks.  Two steps, each a child process of its
own under a time limit; the second starts only when the first ended well:
  device      --rounds rounds of Batch.components followed by Batch.defect_table + download_defect_table:
              on the run's defect maps at 6 neighbours without and with the signal columns, at max_rows
              64 and 1024; on the masks; and on the two extremes, an all-ones map (every voxel of a study
              in one row: the contention case) and the checkerboard at 4 neighbours (50 M components of
              one voxel: the selection case).  Per case the dtab_b kernel class with the bytes its sweep
              has to move (root 4 + size 4, and x 4 with the signal, per voxel) and their share of the 8
              TB/s HBM spec, comp_b of the labelling before it in the same round, and the host clock
              from the enqueue to the table on the host.
  host-route  what a caller does without it: download_components -> scipy.ndimage.find_objects and the
              sums per component (np.bincount over the labels) on --host-studies studies, host clock,
              scaled to the batch by the study count (an estimate); the sizes, sums and boxes of those
              studies are asserted equal to the device's rows outside the timed window.
Prints one JSON line per step; with --out also writes both into that file (profiles/defect_table.json).
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


def table_rounds(B, rounds, source, conn, min_size, max_rows, norm):
    for _ in range(2):   # warm-up
        B.components(source, conn)
        B.defect_table(min_size, max_rows, norm)
    B.download_defect_table()
    kern, comp, host, nbytes, got = [], [], [], 0.0, None
    for _ in range(rounds):
        B.reset_timers()
        B.components(source, conn)
        B.sync()
        t0 = time.perf_counter()
        B.defect_table(min_size, max_rows, norm)
        got = B.download_defect_table()
        host.append(time.perf_counter() - t0)
        ms, n, nbytes = B.kernel_time("dtab_b")
        assert n == 1, n
        kern.append(ms)
        ms, n, _ = B.kernel_time("comp_b")
        assert n == 1, n
        comp.append(ms)
    kk = stats(kern, 1e3, "us")
    gbs = nbytes / (kk["median_us"] * 1e-6) / 1e9
    st = got["stats"]
    return {"source": source, "conn": conn, "min_size": min_size, "max_rows": max_rows, "norm": norm,
            "dtab_b_us": kk, "comp_b_us_same_rounds": stats(comp, 1e3, "us"),
            "dtab_over_comp": round(kk["median_us"] / float(np.median(comp) * 1e3), 3),
            "sweep_bytes_per_launch": nbytes, "achieved_GBps": round(gbs, 1),
            "share_of_hbm_spec": round(gbs / HBM_PEAK_GBS, 4),
            "enqueue_to_table_host_ms": stats(host, 1e3, "ms"), "table_bytes_to_host": int(got["rows"].nbytes),
            "rows_total": int(st[:, 0].sum()), "qualifying_total": int(st[:, 1].sum()),
            "voxels_in_rows_total": int(st[:, 2].sum()), "studies_truncated": int(got["truncated"].sum())}


def step_device(args):
    B, hp, mk = bench_batch(args)
    defect = B.download_defect()[0].copy()
    out = {"what": "defect_table", "step": "device", "shape": list(args.shape), "batch": args.batch,
           "rounds": args.rounds, "defect_fraction": round(float((defect != 0).mean()), 4),
           "masked_fraction": round(float((mk != 0).mean()), 4)}
    out["bench_defect_maps_conn6"] = [table_rounds(B, args.rounds, "defect", 6, 1, n, norm)
                                      for norm in (None, "mean") for n in (64, 1024)]
    out["bench_masks_conn6"] = [table_rounds(B, args.rounds, "mask", 6, 1, 64, norm) for norm in (None, "mean")]
    B.upload_defect(np.ones_like(defect))
    out["all_ones_conn6"] = [table_rounds(B, args.rounds, "defect", 6, 1, 64, norm) for norm in (None, "mean")]
    rr, cc = np.mgrid[0:args.shape[0], 0:args.shape[1]]
    B.upload_defect(np.broadcast_to((((rr + cc) % 2) == 0)[None, :, :, None], defect.shape))
    out["checkerboard_conn4"] = [table_rounds(B, args.rounds, "defect", 4, 1, n, None) for n in (64, 1024)]
    B.close()
    print(json.dumps(out))


def host_table(root):
    """One study on the host from its root map: per component the size, the index sums and the box."""
    from scipy import ndimage as ndi
    roots, lab = np.unique(root[root >= 0], return_inverse=True)
    labels = np.zeros(root.shape, np.int32)
    labels[root >= 0] = lab + 1
    boxes = ndi.find_objects(labels)
    flat = labels.ravel()
    n = len(roots) + 1
    idx = np.unravel_index(np.arange(flat.size), root.shape)
    size = np.bincount(flat, minlength=n)[1:]
    sums = [np.bincount(flat, weights=i, minlength=n)[1:].astype(np.int64) for i in idx]
    return roots, size, sums, boxes


def step_host_route(args):
    B, hp, mk = bench_batch(args)
    n = min(args.host_studies, args.batch)
    B.components("defect", 6)
    ts = {"download_components": [], "find_objects_and_sums": []}
    host = None
    for _ in range(args.host_rounds):
        t0 = time.perf_counter()
        cc = B.download_components()
        t1 = time.perf_counter()
        host = [host_table(cc["root"][q]) for q in range(n)]
        t2 = time.perf_counter()
        ts["download_components"].append(t1 - t0)
        ts["find_objects_and_sums"].append(t2 - t1)
    B.defect_table(1, 1024)   # parity at the timed size
    got = B.download_defect_table()
    equal = True
    for q in range(n):
        roots, size, sums, boxes = host[q]
        rows = got["rows"][q][:got["stats"][q, 0]]
        at = np.searchsorted(roots, rows[:, 0])
        equal = equal and not got["truncated"][q] and len(rows) == len(roots)
        equal = equal and np.array_equal(rows[:, 1], size[at]) and all(np.array_equal(rows[:, 2 + a], sums[a][at]) for a in range(3))
        equal = equal and all(rows[j, 5 + 2 * a] == boxes[at[j]][a].start and rows[j, 6 + 2 * a] == boxes[at[j]][a].stop - 1
                              for j in range(len(rows)) for a in range(3))
    assert equal
    per_study = float(np.median(ts["find_objects_and_sums"])) / n
    total = float(np.median(ts["download_components"])) + per_study * args.batch
    out = {"what": "defect_table", "step": "host-route", "shape": list(args.shape), "batch": args.batch,
           "rounds": args.host_rounds, "studies_on_the_host": n, "equal_to_the_device_result": bool(equal),
           "parts_host_ms": {q: stats(v, 1e3, "ms") for q, v in ts.items()},
           "scipy_and_numpy_ms_per_study": round(per_study * 1e3, 3),
           "download_scipy_host_ms_scaled_to_the_batch_estimate": round(total * 1e3, 1)}
    B.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--shape", type=int, nargs=3, default=(128, 128, 24))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--host-rounds", type=int, default=2, help="rounds of the host route")
    ap.add_argument("--host-studies", type=int, default=4, help="studies the host route tabulates")
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
            json.dump({"what": "defect_table", "script": "scripts/defect_table_bench.py", "device": "one MI355X",
                       "this_change": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
