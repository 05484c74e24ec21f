#!/usr/bin/env python3
"""The proton-to-xenon registration on the device-resident bench batch, timed against numpy.

Inputs: bench.py's batch size (256 x 128x128x24).  The pair of a study is the synthetic phantom of
tests/register_ref.py (a bright body with two dark lungs that vary with the slice in the proton, the
xenon bright in the lungs, Rician-like noise), the proton displaced by a planted shift that differs from
study to study; --unique studies are generated and repeated through the batch.  Three steps, each a child
process of its own under a time limit; the next starts only when the last ended well:
  device       the noisy phantom: Batch.register at search (4, 4, 1) and (8, 8, 2).  Two warm-up calls,
               then --rounds rounds: host clock from the enqueue to the scores and picks on the host, and
               the kernel classes register_b (the joint histograms), register_score_b, register_codes_b
               and segment_max_b (the two maximum sweeps) per call; voxel-shift pairs per second of
               register_b; Batch.shift_proton's class shift_b.  The picks that equal the planted shifts
               are counted outside the timed window.
  device-zero  the same on the variant whose background is exactly 0 in both images, so that bin (0, 0)
               holds most pairs of every shift.
  host-route   the same search in numpy (register_ref: slicing and np.bincount per shift, mi in
               float64) on --host-studies studies, scaled to the batch by the study count; its picks and
               scores are compared with the device's outside the timed window.
Prints one JSON line per step and writes them to --out (profiles/register.json), with a last line that
holds the ratio of register_b on the zero-background variant to the noisy one.
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
SEARCHES = ((4, 4, 1), (8, 8, 2))
CLASSES = ("register_b", "register_score_b", "register_codes_b", "segment_max_b")


def stats(ts, scale, unit):
    ts = np.asarray(ts) * scale
    return {"median_" + unit: round(float(np.median(ts)), 4), "min_" + unit: round(float(ts.min()), 4),
            "max_" + unit: round(float(ts.max()), 4), "n": int(ts.size)}


def planted_shift(q):
    """Inside the smaller window, different from study to study."""
    return (q * 3) % 9 - 4, (q * 5 + 2) % 9 - 4, q % 3 - 1


def phantom(args, kind):
    """(proton, xenon) float32 [batch][R][C][Z] and the planted shifts int32 [batch][3]."""
    import register_ref as G
    shape = tuple(args.shape)
    pairs = [G.study(shape, planted_shift(q), kind, 500 + q) for q in range(args.unique)]
    idx = np.arange(args.batch) % args.unique
    P = np.stack([pairs[i][0] for i in idx])
    X = np.stack([pairs[i][1] for i in idx])
    return P, X, np.array([planted_shift(i) for i in idx], np.int32)


def resident(args, kind):
    from vent_analysis_amd import _lib
    R, C, Z = args.shape
    P, X, planted = phantom(args, kind)
    B = _lib.Batch(R, C, Z, args.batch)
    B.upload(X, np.ones(X.shape, np.uint8))
    B.run(B.options(do_n4=False, do_kmeans=False, vox=VOX, profile=True))   # (turns the kernel timers on)
    B.sync()
    B.upload_proton(P)
    return B, P, X, planted


def timed_register(B, search, rounds, voxels):
    for _ in range(2):
        best, score, status = B.register(search)
    host, kern = [], {c: [] for c in CLASSES}
    for _ in range(rounds):
        B.reset_timers()
        t0 = time.perf_counter()
        best, score, status = B.register(search)
        host.append(time.perf_counter() - t0)
        for c in CLASSES:
            ms, launches, _ = B.kernel_time(c)
            kern[c].append(ms / max(1, launches))
    ns = score[0].size
    out = {"shifts": int(ns), "enqueue_to_scores_host_ms": stats(host, 1e3, "ms")}
    for c in CLASSES:
        out[c + "_ms_per_launch"] = stats(kern[c], 1.0, "ms")
    pairs = float(voxels) * ns
    out["voxel_shift_pairs"] = pairs
    out["pairs_per_second_of_register_b"] = float("%.4g" % (pairs / (out["register_b_ms_per_launch"]["median_ms"] * 1e-3)))
    out["joint_histogram_bytes"] = int(score.shape[0]) * int(ns) * 4096
    return out, best, score


def step_device(args, kind):
    B, P, X, planted = resident(args, kind)
    out = {"what": "register", "step": "device" if kind == 0 else "device-zero", "shape": list(args.shape),
           "batch": args.batch, "unique_studies": args.unique, "rounds": args.rounds,
           "background": "Rician-like noise" if kind == 0 else "exactly 0 in both images", "settings": {}}
    for search in SEARCHES:
        res, best, score = timed_register(B, search, args.rounds, P.size)
        res["picks_equal_to_the_planted_shifts"] = int((best == planted).all(axis=1).sum())
        if search == SEARCHES[0]:
            h = B.register(search, hist=True)[3]
            centre = h[:, 1, 4, 4]
            res["largest_share_of_one_bin_at_shift_0"] = round(float((centre.reshape(len(h), -1).max(axis=1) /
                                                                      centre.reshape(len(h), -1).sum(axis=1)).mean()), 4)
            np.save(os.path.join(args.scratch, "register_kind%d.npy" % kind), score[:args.host_studies])
        out["settings"]["search_%d_%d_%d" % search] = res
    ts = []
    for _ in range(args.rounds):
        B.reset_timers()
        B.shift_proton(planted)
        B.sync()
        ts.append(B.kernel_time("shift_b")[0])
    out["shift_b_ms_per_launch"] = stats(ts, 1.0, "ms")
    B.close()
    print(json.dumps(out))


def step_host_route(args):
    import register_ref as G
    P, X, planted = phantom(args, 0)
    n = min(args.host_studies, args.batch)
    search = SEARCHES[0]
    t0 = time.perf_counter()
    hist, score, best, gaps = G.reference_of(P[:n], X[:n], search)
    t1 = time.perf_counter()
    dev = np.load(os.path.join(args.scratch, "register_kind0.npy"))[:n].reshape(n, -1)
    err = float(np.abs(dev - score).max())
    equal = [tuple(b) for b in best] == [tuple(p) for p in planted[:n].tolist()]
    assert equal and err <= 1e-10, (best, err)
    per_study = (t1 - t0) / n
    out = {"what": "register", "step": "host-route", "shape": list(args.shape), "batch": args.batch,
           "search": list(search), "studies_registered_in_numpy": n, "numpy_ms_per_study": round(per_study * 1e3, 1),
           "numpy_host_ms_scaled_to_the_batch": round(per_study * args.batch * 1e3, 0),
           "picks_equal_the_planted_shifts": equal, "largest_score_difference_to_the_device": err,
           "smallest_gap_to_the_second_best_score": round(min(gaps), 5)}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--shape", type=int, nargs=3, default=(128, 128, 24))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--unique", type=int, default=16, help="phantom studies generated and repeated through the batch")
    ap.add_argument("--host-studies", type=int, default=2, help="studies the host route registers in numpy")
    ap.add_argument("--step", choices=("device", "device-zero", "host-route"), help="run this one step in this process")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per step")
    ap.add_argument("--scratch", default=None, help="where the device step leaves its scores for the host route")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "register.json"))
    args = ap.parse_args()
    if args.rounds < 1 or args.host_studies < 1 or args.unique < 1:
        sys.exit("--rounds, --unique and --host-studies must be >= 1")
    args.host_studies = min(args.host_studies, args.unique)
    if args.step:
        {"device": lambda a: step_device(a, 0), "device-zero": lambda a: step_device(a, 1),
         "host-route": step_host_route}[args.step](args)
        return
    import tempfile
    lines = []
    with tempfile.TemporaryDirectory() as scratch:
        for step in ("device", "device-zero", "host-route"):   # chained: a failed or hung step ends the script
            cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--batch", str(args.batch),
                   "--rounds", str(args.rounds), "--host-studies", str(args.host_studies), "--unique", str(args.unique),
                   "--scratch", scratch, "--shape", *map(str, args.shape)]
            try:
                p = subprocess.run(cmd, timeout=args.timeout, stdout=subprocess.PIPE, text=True)
            except subprocess.TimeoutExpired:
                sys.exit(f"step {step}: no end after {args.timeout} s; nothing further started")
            sys.stdout.write(p.stdout)
            if p.returncode != 0:
                sys.exit(f"step {step} ended with status {p.returncode}; nothing further started")
            lines.append(p.stdout.strip().splitlines()[-1])
    noisy, zero = (json.loads(l)["settings"] for l in lines[:2])
    ratio = {k: round(zero[k]["register_b_ms_per_launch"]["median_ms"] / noisy[k]["register_b_ms_per_launch"]["median_ms"], 3)
             for k in noisy}
    last = {"what": "register", "step": "hot-bin", "register_b_zero_background_over_noisy": ratio,
            "at_most_2": all(v <= 2.0 for v in ratio.values())}
    print(json.dumps(last))
    lines.append(json.dumps(last))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
