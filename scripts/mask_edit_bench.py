#!/usr/bin/env python3
"""The mask edits on the device-resident bench batch, timed against what they replace.

Inputs: bench.py's default batch (256 x 128x128x24, synth_batch base_seed 0, 64 unique studies,
vary=True) and its masks.  Two steps, each a child process of its own under a time limit; the second
starts only when the first ended well:
  device      per op (erode, dilate, open, close) and radius (1, 3, 5), and for the OR paint: the
              masks are uploaded again, two warm-up calls, then --rounds rounds of Batch.edit_mask
              (Batch.paint_mask) followed by Batch.download_mask, host clock from the enqueue to the
              downloaded mask, and the mask_edit_b kernel class of the same call: milliseconds per call
              (open and close are two launches of the one kernel) and the share of the 8 TB/s HBM spec
              on the 2 nb V bytes a pass has to move.  The kernel has no data-dependent work, so a
              round that edits the previous round's output takes the same time.
  host-route  what a caller does without it: Batch.download_mask -> scipy.ndimage per study ->
              Batch.upload, host clock, on --host-studies studies and scaled to the batch by the study
              count; the result of those studies is asserted equal to the device's, byte for byte,
              outside the timed window.
Prints one JSON line per step and writes both to --out (profiles/mask_edit.json).
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
OPS = ("erode", "dilate", "open", "close")
RADII = (1, 3, 5)
HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec, as bench.py


def stats(ts, scale, unit):
    ts = np.asarray(ts) * scale
    return {"median_" + unit: round(float(np.median(ts)), 4), "min_" + unit: round(float(ts.min()), 4),
            "max_" + unit: round(float(ts.max()), 4), "n": int(ts.size)}


def bench_batch(args):
    from vent_analysis_amd import _lib
    from vent_analysis_amd.synth import synth_batch
    R, C, Z = args.shape
    hp, mk = synth_batch(R, C, Z, args.batch, base_seed=0, unique=64, vary=True)
    mk = np.ascontiguousarray(mk, dtype=np.uint8)
    B = _lib.Batch(R, C, Z, args.batch)
    B.upload(hp, mk)
    return B, mk


def strokes_for(mk):
    """A few painted voxels per study: one voxel in 500."""
    rng = np.random.default_rng(3)
    return (rng.random(mk.shape, dtype=np.float32) < 0.002).astype(np.uint8)


def timed(B, call, rounds):
    host, kern, launches, nbytes = [], [], 0, 0.0
    for _ in range(rounds):
        B.reset_timers()
        t0 = time.perf_counter()
        call()
        B.download_mask()
        host.append(time.perf_counter() - t0)
        ms, launches, nbytes = B.kernel_time("mask_edit_b")
        kern.append(ms)
    k = stats(kern, 1.0, "ms")
    gbs = nbytes * launches / (k["median_ms"] * 1e-3) / 1e9
    return {"enqueue_to_download_mask_host_ms": stats(host, 1e3, "ms"), "mask_edit_b_ms_per_call": k,
            "launches_per_call": int(launches), "bytes_moved_per_launch": nbytes,
            "achieved_GBps": round(gbs, 1), "share_of_hbm_spec": round(gbs / HBM_PEAK_GBS, 4)}


def step_device(args):
    B, mk = bench_batch(args)
    B.run(B.options(do_n4=False, do_kmeans=False, vox=VOX, profile=True))   # (turns the kernel timers on)
    B.sync()
    out = {"what": "mask_edit", "step": "device", "shape": list(args.shape), "batch": args.batch,
           "rounds": args.rounds, "hbm_spec_GBps": HBM_PEAK_GBS, "settings": {}}
    B.download_mask()   # (warm-up: the first call allocates the page-locked host buffer)
    ts = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        B.download_mask()
        ts.append(time.perf_counter() - t0)
    out["download_mask_alone_host_ms"] = stats(ts, 1e3, "ms")
    for op in OPS:
        for r in RADII:
            B.upload(None, mk)
            for _ in range(2):
                B.edit_mask(op, r)
            B.sync()
            out["settings"]["%s_r%d" % (op, r)] = timed(B, lambda: B.edit_mask(op, r), args.rounds)
    st = strokes_for(mk)
    B.upload(None, mk)
    for _ in range(2):
        B.paint_mask(st, "or")
    B.sync()
    out["settings"]["paint_or"] = timed(B, lambda: B.paint_mask(st, "or"), args.rounds)
    B.close()
    print(json.dumps(out))


def step_host_route(args):
    import scipy.ndimage as ndi
    B, mk = bench_batch(args)
    n = min(args.host_studies, args.batch)
    out = {"what": "mask_edit", "step": "host-route", "shape": list(args.shape), "batch": args.batch,
           "studies_edited_in_scipy": n, "settings": {}}

    def host_edit(s, op, d):
        st = d[:, :, None]
        dil = lambda a: ndi.binary_dilation(a, structure=st)                    # noqa: E731
        ero = lambda a: ndi.binary_erosion(a, structure=st, border_value=1)     # noqa: E731
        return {"erode": ero, "dilate": dil, "open": lambda a: dil(ero(a)), "close": lambda a: ero(dil(a))}[op](s)

    for op in OPS:
        for r in RADII:
            rr, cc = np.mgrid[-r:r + 1, -r:r + 1]
            d = rr * rr + cc * cc <= r * r
            B.upload(None, mk)
            t0 = time.perf_counter()
            x = B.download_mask()
            t1 = time.perf_counter()
            ref = [host_edit(x[q] != 0, op, d).astype(np.uint8) for q in range(n)]
            t2 = time.perf_counter()
            B.upload(None, x)
            t3 = time.perf_counter()
            B.edit_mask(op, r)   # parity at the timed size
            got = B.download_mask()
            equal = all(np.array_equal(got[q], ref[q]) for q in range(n))
            assert equal, (op, r)
            per_study = (t2 - t1) / n
            out["settings"]["%s_r%d" % (op, r)] = {
                "download_mask_host_ms": round((t1 - t0) * 1e3, 3), "upload_host_ms": round((t3 - t2) * 1e3, 3),
                "scipy_ms_per_study": round(per_study * 1e3, 3), "equal_to_the_device_result": equal,
                "download_scipy_upload_host_ms_scaled_to_the_batch":
                    round(((t1 - t0) + per_study * args.batch + (t3 - t2)) * 1e3, 1)}
    B.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--shape", type=int, nargs=3, default=(128, 128, 24))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--host-studies", type=int, default=16, help="studies the host route edits in scipy")
    ap.add_argument("--step", choices=("device", "host-route"), help="run this one step in this process")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per step")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mask_edit.json"))
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
