#!/usr/bin/env python3
"""The proton resampled onto the xenon grid of the device-resident bench batch, timed against numpy.

Inputs: bench.py's batch (256 studies of 128x128x24) as the destination, and a proton of 256x256x24 per
study -- the synthetic phantom of tests/resample_ref.py at half the pixel size -- at the map (2, 0.5),
(2, 0.5), (1, 0); --unique studies are generated and repeated through the batch.  Two steps, each a child
process of its own under a time limit; the next starts only when the last ended well:
  device       Batch.upload_proton_src timed on the host clock (it returns once the source is on the
               device), then for every LDS budget of --lds-kb (0: the library's default) two warm-up calls
               and --rounds rounds of Batch.resample_proton: the kernel class resample_b from
               vh_batch_kernel_time, and the host clock from the enqueue to the end of the stream; the bytes
               the kernel has to move (the source read once, the destination written once) over the kernel
               time, as a fraction of the 8 TB/s HBM spec.  The first --host-studies studies are compared
               with the reference by bytes outside the timed window, at every budget.  Last, the kernel class
               at the map whose slice offset is 0.25: two z-taps per slice.
  host-route   the same resampling in numpy (resample_ref: three vectorised float32 passes) on
               --host-studies studies, scaled to the batch by the study count.
Prints one JSON line per step and writes them to --out (profiles/resample.json), in place of the lines of
these two steps there; lines of other steps in that file are kept.
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
MAP = [[2.0, 0.5], [2.0, 0.5], [1.0, 0.0]]
MAP_Z = [[2.0, 0.5], [2.0, 0.5], [1.0, 0.25]]   # a quarter slice off: two z-taps
OWN_STEPS = ("device", "host-route")
HBM_SPEC = 8e12


def stats(ts, scale, unit):
    ts = np.asarray(ts) * scale
    return {"median_" + unit: round(float(np.median(ts)), 4), "min_" + unit: round(float(ts.min()), 4),
            "max_" + unit: round(float(ts.max()), 4), "n": int(ts.size)}


def phantom(args):
    import resample_ref as F
    uniq = [F.study(tuple(args.src_shape), 900 + q) for q in range(args.unique)]
    return np.stack([uniq[i % args.unique] for i in range(args.batch)])


def step_device(args):
    import resample_ref as F
    from vent_analysis_amd import _lib
    src = phantom(args)
    R, C, Z = args.shape
    n = min(args.host_studies, args.batch)
    want = F.reference_of(src[:n], [MAP] * n, (R, C, Z))
    B = _lib.Batch(R, C, Z, args.batch)
    B.upload(np.zeros((args.batch, R, C, Z), np.float32), np.ones((args.batch, R, C, Z), np.uint8))
    B.run(B.options(do_n4=False, do_kmeans=False, vox=VOX, profile=True))   # (turns the kernel timers on)
    B.sync()
    up = []
    for _ in range(3):
        t0 = time.perf_counter()
        B.upload_proton_src(src)
        up.append(time.perf_counter() - t0)
    moved = 4.0 * (src.size + args.batch * R * C * Z)
    out = {"what": "resample", "step": "device", "src_shape": list(args.src_shape), "shape": [R, C, Z],
           "batch": args.batch, "unique_studies": args.unique, "rounds": args.rounds, "map": MAP,
           "upload_proton_src_host_ms": stats(up, 1e3, "ms"), "source_bytes": int(src.nbytes),
           "bytes_the_kernel_moves": int(moved), "lds_budget_kb": {}}
    for kb in args.lds_kb:
        if kb:
            os.environ["VH_RS_LDS_KB"] = str(kb)
        else:
            os.environ.pop("VH_RS_LDS_KB", None)
        for _ in range(2):
            B.resample_proton(MAP)
        B.sync()
        host, kern = [], []
        for _ in range(args.rounds):
            B.reset_timers()
            t0 = time.perf_counter()
            B.resample_proton(MAP)
            B.sync()
            host.append(time.perf_counter() - t0)
            ms, launches, _ = B.kernel_time("resample_b")
            kern.append(ms / max(1, launches))
        got = B.download_proton()[:n]
        res = {"resample_b_ms_per_launch": stats(kern, 1.0, "ms"), "enqueue_to_done_host_ms": stats(host, 1e3, "ms"),
               "equal_to_the_reference_by_bytes": bool(got.tobytes() == want.tobytes())}
        t = res["resample_b_ms_per_launch"]["median_ms"] * 1e-3
        res["bytes_per_second"] = float("%.4g" % (moved / t))
        res["fraction_of_the_8_TB_per_s_hbm_spec"] = round(moved / t / HBM_SPEC, 4)
        out["lds_budget_kb"]["default" if not kb else str(kb)] = res
        assert res["equal_to_the_reference_by_bytes"], kb
    # a slice offset that is no whole number gives two z-taps: twice the reads per pair, and the kernel's
    # form for them
    os.environ.pop("VH_RS_LDS_KB", None)
    want_z = F.reference_of(src[:n], [MAP_Z] * n, (R, C, Z))
    for _ in range(2):
        B.resample_proton(MAP_Z)
    B.sync()
    kern = []
    for _ in range(args.rounds):
        B.reset_timers()
        B.resample_proton(MAP_Z)
        B.sync()
        ms, launches, _ = B.kernel_time("resample_b")
        kern.append(ms / max(1, launches))
    equal = bool(B.download_proton()[:n].tobytes() == want_z.tobytes())
    out["two_z_taps"] = {"map": MAP_Z, "resample_b_ms_per_launch": stats(kern, 1.0, "ms"),
                         "equal_to_the_reference_by_bytes": equal}
    assert equal
    B.close()
    print(json.dumps(out))


def step_host_route(args):
    import resample_ref as F
    src = phantom(args)
    n = min(args.host_studies, args.batch)
    t0 = time.perf_counter()
    F.reference_of(src[:n], [MAP] * n, tuple(args.shape))
    per_study = (time.perf_counter() - t0) / n
    out = {"what": "resample", "step": "host-route", "src_shape": list(args.src_shape), "shape": list(args.shape),
           "batch": args.batch, "studies_resampled_in_numpy": n, "numpy_ms_per_study": round(per_study * 1e3, 1),
           "numpy_host_ms_scaled_to_the_batch": round(per_study * args.batch * 1e3, 0)}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--shape", type=int, nargs=3, default=(128, 128, 24))
    ap.add_argument("--src-shape", type=int, nargs=3, default=(256, 256, 24))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--unique", type=int, default=8, help="phantom studies generated and repeated through the batch")
    ap.add_argument("--host-studies", type=int, default=2, help="studies the host route resamples in numpy")
    ap.add_argument("--lds-kb", type=int, nargs="+", default=(0, 16, 24, 32, 48, 64),
                    help="LDS budgets (VH_RS_LDS_KB) to time; 0 is the library's default")
    ap.add_argument("--step", choices=("device", "host-route"), help="run this one step in this process")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per step")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "resample.json"))
    args = ap.parse_args()
    if args.rounds < 1 or args.host_studies < 1 or args.unique < 1:
        sys.exit("--rounds, --unique and --host-studies must be >= 1")
    args.host_studies = min(args.host_studies, args.unique)
    if args.step:
        {"device": step_device, "host-route": step_host_route}[args.step](args)
        return
    lines = []
    for step in ("device", "host-route"):   # chained: a failed or hung step ends the script
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--batch", str(args.batch),
               "--rounds", str(args.rounds), "--host-studies", str(args.host_studies), "--unique", str(args.unique),
               "--shape", *map(str, args.shape), "--src-shape", *map(str, args.src_shape),
               "--lds-kb", *map(str, args.lds_kb)]
        try:
            p = subprocess.run(cmd, timeout=args.timeout, stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            sys.exit(f"step {step}: no end after {args.timeout} s; nothing further started")
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            sys.exit(f"step {step} ended with status {p.returncode}; nothing further started")
        lines.append(p.stdout.strip().splitlines()[-1])
    # lines of other steps that --out already holds (the first form's timings, bench.py's headline beside
    # the parent's: measured by hand) are kept
    kept = []
    if os.path.exists(args.out):
        for l in open(args.out).read().splitlines():
            try:
                if l.strip() and json.loads(l).get("step") not in OWN_STEPS:
                    kept.append(l)
            except ValueError:
                pass
    with open(args.out, "w") as f:
        f.write("\n".join(lines + kept) + "\n")


if __name__ == "__main__":
    main()
