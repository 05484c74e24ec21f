#!/usr/bin/env python3
"""The proton segmentation on the device-resident bench batch, timed against what it replaces.

Inputs: bench.py's default batch (256 x 128x128x24, synth_batch base_seed 0, 64 unique studies,
vary=True); the proton of a study is made from its mask: a bright box (100, Gaussian noise of 8) two
pixels inside the image, the lungs (the mask inside the box) and the background Rician noise of 5, three
bright vessel pixels and four dark specks per slice.  Two steps, each a child process of its own under a
time limit; the second starts only when the first ended well:
  device      Batch.upload_proton (host clock); Batch.proton_threshold (host clock, and its two sweeps,
              classes segment_max_b and segment_hist_b, which read 4 nb V bytes each); Batch.segment at open_radius 0 and 1
              followed by Batch.download_mask: host clock from the enqueue to the mask on the host, the
              fill's class segment_b (4 nb V bytes read, nb V written) and the opening's mask_edit_b; the
              fill again with VH_SEG_ZC forcing narrower bit fields (more, smaller workgroups).  Two
              warm-up calls, then --rounds rounds; the fill's rounds depend on the data, not on the call.
  host-route  what a caller does without it, proton on the host: numpy maximum and histogram, the Otsu
              cut, scipy.ndimage.binary_fill_holes per slice, erosion and dilation by the radius-1 disc,
              Batch.upload; host clock, on --host-studies studies and scaled to the batch by the study
              count; the result of those studies is asserted equal to the device's, byte for byte,
              outside the timed window.
Prints one JSON line per step and writes both to --out (profiles/segment.json).
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
    return {"median_" + unit: round(float(np.median(ts)), 4), "min_" + unit: round(float(ts.min()), 4),
            "max_" + unit: round(float(ts.max()), 4), "n": int(ts.size)}


def proton_of(mk):
    """float32 [n][R][C][Z] from the masks uint8 [n][R][C][Z], seeded."""
    rng = np.random.default_rng(17)
    n, R, C, Z = mk.shape
    box = np.zeros((R, C, 1), bool)
    box[2:R - 2, 2:C - 2] = True
    out = np.empty(mk.shape, np.float32)
    cache = {}
    for q in range(n):
        key = mk[q].tobytes()
        if key not in cache:
            lungs = (mk[q] != 0) & box
            x = np.where(box & ~lungs, 100 + rng.normal(0, 8, (R, C, Z)),
                         np.hypot(rng.normal(0, 5, (R, C, Z)), rng.normal(0, 5, (R, C, Z))))
            for z in range(Z):
                for sel, val, cnt in ((lungs[:, :, z], 100.0, 3), ((box[:, :, 0] & ~lungs[:, :, z]), 1.0, 4)):
                    at = np.argwhere(sel)
                    if len(at):
                        for r, c in at[rng.choice(len(at), min(cnt, len(at)), replace=False)]:
                            x[r, c, z] = val
            cache[key] = x.astype(np.float32)
        out[q] = cache[key]
    return out


def bench_batch(args):
    from vent_analysis_amd import _lib
    from vent_analysis_amd.synth import synth_batch
    R, C, Z = args.shape
    hp, mk = synth_batch(R, C, Z, args.batch, base_seed=0, unique=64, vary=True)
    mk = np.ascontiguousarray(mk, dtype=np.uint8)
    B = _lib.Batch(R, C, Z, args.batch)
    B.upload(hp, mk)
    return B, mk, proton_of(mk)


def timed_segment(B, th, radius, rounds):
    for _ in range(2):
        B.segment(th, radius)
    B.sync()
    host, fill, morph, nbytes = [], [], [], 0.0
    for _ in range(rounds):
        B.reset_timers()
        t0 = time.perf_counter()
        B.segment(th, radius)
        B.download_mask()
        host.append(time.perf_counter() - t0)
        ms, _, nbytes = B.kernel_time("segment_b")
        fill.append(ms)
        morph.append(B.kernel_time("mask_edit_b")[0])
    k = stats(fill, 1.0, "ms")
    gbs = nbytes / (k["median_ms"] * 1e-3) / 1e9
    return {"enqueue_to_download_mask_host_ms": stats(host, 1e3, "ms"), "segment_b_ms_per_call": k,
            "mask_edit_b_ms_per_call": stats(morph, 1.0, "ms"), "bytes_moved_by_the_fill": nbytes,
            "fill_GBps": round(gbs, 1), "fill_share_of_hbm_spec": round(gbs / HBM_PEAK_GBS, 4)}


def step_device(args):
    B, mk, proton = bench_batch(args)
    B.run(B.options(do_n4=False, do_kmeans=False, vox=VOX, profile=True))   # (turns the kernel timers on)
    B.sync()
    out = {"what": "segment", "step": "device", "shape": list(args.shape), "batch": args.batch,
           "rounds": args.rounds, "hbm_spec_GBps": HBM_PEAK_GBS, "proton_bytes": int(proton.nbytes)}
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        B.upload_proton(proton)
        ts.append(time.perf_counter() - t0)
    out["upload_proton_host_ms_pageable"] = stats(ts, 1e3, "ms")
    B.download_mask()   # (warm-up: the first call allocates the page-locked host buffer)
    for _ in range(2):
        th = B.proton_threshold()
    host, kmax, khist, nbytes = [], [], [], 0.0
    for _ in range(args.rounds):
        B.reset_timers()
        t0 = time.perf_counter()
        th = B.proton_threshold()
        host.append(time.perf_counter() - t0)
        kmax.append(B.kernel_time("segment_max_b")[0])
        ms, _, nbytes = B.kernel_time("segment_hist_b")
        khist.append(ms)
    out["proton_threshold"] = {"host_ms": stats(host, 1e3, "ms"), "bytes_read_per_sweep": nbytes,
                               "thresholds_min_max": [float(th.min()), float(th.max())]}
    for name, ts in (("segment_max_b", kmax), ("segment_hist_b", khist)):
        k = stats(ts, 1.0, "ms")
        gbs = nbytes / (k["median_ms"] * 1e-3) / 1e9
        out["proton_threshold"][name] = dict(k, achieved_GBps=round(gbs, 1),
                                             share_of_hbm_spec=round(gbs / HBM_PEAK_GBS, 4))
    out["settings"] = {}
    for radius in (0, 1):
        out["settings"]["open_r%d" % radius] = timed_segment(B, th, radius, args.rounds)
    got, cnt = B.download_mask(count=True)
    out["voxels_segmented_min_max"] = [int(cnt.min()), int(cnt.max())]
    ov = B.mask_overlap(mk)
    out["dice_against_the_bench_masks_min_max"] = [round(float(v), 4) for v in
                                                   (lambda d: (d.min(), d.max()))(2 * ov[:, 2] / (ov[:, 0] + ov[:, 1]))]
    for zc in (16, 8, 4):
        os.environ["VH_SEG_ZC"] = str(zc)
        out["settings"]["open_r0_VH_SEG_ZC_%d" % zc] = timed_segment(B, th, 0, args.rounds)
    del os.environ["VH_SEG_ZC"]
    B.close()
    print(json.dumps(out))


def step_host_route(args):
    import scipy.ndimage as ndi
    from vent_analysis_amd import _lib
    B, mk, proton = bench_batch(args)
    n = min(args.host_studies, args.batch)
    disc = ndi.generate_binary_structure(2, 1)[:, :, None]
    t0 = time.perf_counter()
    ref, ths = [], []
    for q in range(n):
        x = proton[q]
        f = x[np.isfinite(x) & (x >= 0)]
        pmax = f.max()
        scale = np.float32(256.0) / pmax
        hist = np.bincount(np.minimum(255, (f * scale).astype(np.int64)), minlength=256)
        t = np.float32(_lib.otsu(hist) + 1) * (pmax / np.float32(256.0))
        dark = x < t
        seg = np.stack([ndi.binary_fill_holes(~dark[:, :, z]) for z in range(x.shape[2])], axis=2) & dark
        seg = ndi.binary_dilation(ndi.binary_erosion(seg, structure=disc, border_value=1), structure=disc)
        ref.append(seg.astype(np.uint8))
        ths.append(t)
    t1 = time.perf_counter()
    full = np.ascontiguousarray(np.concatenate([np.stack(ref)] * (args.batch // n + 1))[:args.batch])
    t2 = time.perf_counter()
    B.upload(None, full)
    t3 = time.perf_counter()
    B.upload_proton(proton)   # parity at the timed size
    used = B.segment(open_radius=1)
    got = B.download_mask()
    equal = all(np.array_equal(got[q], ref[q]) for q in range(n)) and used[:n].tolist() == [float(t) for t in ths]
    assert equal
    per_study = (t1 - t0) / n
    out = {"what": "segment", "step": "host-route", "shape": list(args.shape), "batch": args.batch,
           "studies_segmented_on_the_host": n, "open_radius": 1,
           "numpy_scipy_ms_per_study": round(per_study * 1e3, 3), "upload_host_ms": round((t3 - t2) * 1e3, 3),
           "equal_to_the_device_result": equal,
           "numpy_scipy_upload_host_ms_scaled_to_the_batch": round((per_study * args.batch + (t3 - t2)) * 1e3, 1)}
    B.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--shape", type=int, nargs=3, default=(128, 128, 24))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--host-studies", type=int, default=16, help="studies the host route segments in scipy")
    ap.add_argument("--step", choices=("device", "host-route"), help="run this one step in this process")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per step")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "segment.json"))
    args = ap.parse_args()
    if args.rounds < 1 or args.host_studies < 1:
        sys.exit("--rounds and --host-studies must be >= 1")
    if args.step:
        {"device": step_device, "host-route": step_host_route}[args.step](args)
        return
    lines = []
    for step in ("device", "host-route"):   # chained: a failed or hung step ends the script
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--batch", str(args.batch),
               "--rounds", str(args.rounds), "--host-studies", str(args.host_studies),
               "--shape", *map(str, args.shape)]
        try:
            p = subprocess.run(cmd, timeout=args.timeout, stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            sys.exit(f"step {step}: no end after {args.timeout} s; nothing further started")
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            sys.exit(f"step {step} ended with status {p.returncode}; nothing further started")
        lines.append(p.stdout.strip().splitlines()[-1])
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
