#!/usr/bin/env python3
"""The fine registration on the device-resident bench batch, timed against the route it replaces.

Inputs: bench.py's batch size (256 x 128x128x24) with a source proton of 256x256x24 per study.  The pair
of a study is the phantom of tests/register_maps_ref.py: the source a bright body with two dark lungs, the
xenon derived from the source resampled through a planted candidate that differs from study to study;
--unique studies are generated and repeated through the batch.  One step, a child process under a time
limit:
  device   Batch.register_maps at 15 x 15 x 3 = 675 candidates (map_candidates' defaults around the
           centre-on-centre map) and at 3 x 3 x 1.  Two warm-up calls, then --rounds rounds: host clock from
           the enqueue to the scores and picks on the host, and the kernel classes register_maps_b (the
           fused kernel), register_maps_codes_b, register_score_b and segment_max_b per call; voxel-
           candidate pairs per second of register_maps_b, next to the voxel-shift pairs per second of
           register_b (Batch.register at search (4, 4, 1) on the same batch, the proton resampled with the
           base map).  The picks that equal the planted candidates are counted outside the timed window.
           Then the route the search replaces, with the same library: per candidate one
           Batch.resample_proton and one Batch.register((0, 0, 0)), host clock to the score on the host,
           over --route-candidates candidates and scaled to the candidate count (its kernels resample_b
           and register_b are reported per candidate too).  Its scores are not the search's: it codes each
           resampled proton by that volume's own maximum, the search every candidate by the source's.
Prints one JSON line and writes it to --out (profiles/register_maps.json).
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
CLASSES = ("register_maps_b", "register_maps_codes_b", "register_score_b", "segment_max_b")
SMALL = dict(factors=(0.97, 1.0, 1.03), shifts=(0.0,), zshifts=(0.0,))


def stats(ts, scale, unit):
    ts = np.asarray(ts) * scale
    return {"median_" + unit: round(float(np.median(ts)), 4), "min_" + unit: round(float(ts.min()), 4),
            "max_" + unit: round(float(ts.max()), 4), "n": int(ts.size)}


def planted_candidate(q):
    """Inside the 15 x 15 x 3 grid, different from study to study."""
    return (q * 3) % 15, (q * 5 + 2) % 15, q % 3


def phantom(args):
    """(source float32 [batch][Rs][Cs][Zs], xenon float32 [batch][R][C][Z], the base map, the lists, the
    planted candidates int32 [batch][3])."""
    import register_maps_ref as M
    import resample_ref as S
    from vent_analysis_amd import _lib
    src_shape, shape = tuple(args.src_shape), tuple(args.shape)
    base = _lib.grid_map(src_shape, (VOX[0] * shape[0] / src_shape[0], VOX[1] * shape[1] / src_shape[1],
                                     VOX[2] * shape[2] / src_shape[2]), shape, VOX)
    lists, home = _lib.map_candidates(base, shape)
    srcs, xs = [], []
    for q in range(args.unique):
        s = S.study(src_shape, 700 + q)
        k = planted_candidate(q)
        srcs.append(s)
        xs.append(M.xenon_of(s, shape, [lists[0][k[0]], lists[1][k[1]], lists[2][k[2]]], 900 + q).astype(np.float32))
    idx = np.arange(args.batch) % args.unique
    return (np.stack([srcs[i] for i in idx]), np.stack([xs[i] for i in idx]), base, lists, home,
            np.array([planted_candidate(i) for i in idx], np.int32))


def timed_search(B, lists, home, rounds, voxels):
    for _ in range(2):
        best, best_map, score, status = B.register_maps(lists, home)
    host, kern = [], {c: [] for c in CLASSES}
    for _ in range(rounds):
        B.reset_timers()
        t0 = time.perf_counter()
        best, best_map, score, status = B.register_maps(lists, home)
        host.append(time.perf_counter() - t0)
        for c in CLASSES:
            ms, launches, _ = B.kernel_time(c)
            kern[c].append(ms / max(1, launches))
    nc = score[0].size
    out = {"candidates": int(nc), "count": [len(l) for l in lists],
           "enqueue_to_picks_host_ms": stats(host, 1e3, "ms")}
    for c in CLASSES:
        out[c + "_ms_per_launch"] = stats(kern[c], 1.0, "ms")
    pairs = float(voxels) * nc
    out["voxel_candidate_pairs"] = pairs
    out["pairs_per_second_of_register_maps_b"] = float("%.4g" % (pairs / (out["register_maps_b_ms_per_launch"]["median_ms"] * 1e-3)))
    out["joint_histogram_bytes"] = int(score.shape[0]) * int(nc) * 4096
    return out, best, score


def step_device(args):
    from vent_analysis_amd import _lib
    src, X, base, lists, home, planted = phantom(args)
    R, C, Z = args.shape
    B = _lib.Batch(R, C, Z, args.batch)
    B.upload(X, np.ones(X.shape, np.uint8))
    B.run(B.options(do_n4=False, do_kmeans=False, vox=VOX, profile=True))   # (turns the kernel timers on)
    B.sync()
    B.upload_proton_src(src)
    out = {"what": "register_maps", "step": "device", "src_shape": list(args.src_shape), "shape": list(args.shape),
           "batch": args.batch, "unique_studies": args.unique, "rounds": args.rounds, "settings": {}}
    res, best, score = timed_search(B, lists, home, args.rounds, X.size)
    res["picks_equal_to_the_planted_candidates"] = int((best == planted).all(axis=1).sum())
    out["settings"]["15x15x3"] = res
    small, shome = _lib.map_candidates(base, args.shape, **SMALL)
    out["settings"]["3x3x1"] = timed_search(B, small, shome, args.rounds, X.size)[0]

    # register_b on the same batch, for its pairs per second
    B.resample_proton(base)
    search = (4, 4, 1)
    for _ in range(2):
        B.register(search)
    ts = []
    for _ in range(args.rounds):
        B.reset_timers()
        B.register(search)
        ts.append(B.kernel_time("register_b")[0])
    ns = 9 * 9 * 3
    med = float(np.median(ts))
    out["register_b_at_search_4_4_1"] = {"shifts": ns, "register_b_ms_per_launch": stats(ts, 1.0, "ms"),
                                         "pairs_per_second_of_register_b": float("%.4g" % (X.size * ns / (med * 1e-3)))}

    # the route the search replaces: one resampling and one single-shift registration per candidate
    n = min(args.route_candidates, score[0].size)
    pick = np.linspace(0, score[0].size - 1, n).astype(int)
    cand = [(int(i // 15 % 15), int(i % 15), int(i // 225)) for i in pick]
    host, kr, kg = [], [], []
    for w, (a, b, c) in enumerate([cand[0]] + cand):                        # (the first once more as a warm-up)
        m = np.asarray([lists[0][a], lists[1][b], lists[2][c]])
        B.reset_timers()
        t0 = time.perf_counter()
        B.resample_proton(m)
        B.register((0, 0, 0))
        dt = time.perf_counter() - t0
        if w == 0:
            continue
        host.append(dt)
        kr.append(B.kernel_time("resample_b")[0])
        kg.append(B.kernel_time("register_b")[0])
    nc = score[0].size
    out["replaced_route"] = {
        "what": "per candidate Batch.resample_proton + Batch.register((0, 0, 0)), host clock to the score on the host",
        "candidates_measured": n, "scaled_to_candidates": int(nc),
        "host_ms_per_candidate": stats(host, 1e3, "ms"),
        "resample_b_ms_per_candidate": stats(kr, 1.0, "ms"), "register_b_ms_per_candidate": stats(kg, 1.0, "ms"),
        "host_ms_scaled": round(float(np.median(host)) * 1e3 * nc, 1),
        "kernels_ms_scaled": round(float(np.median(kr) + np.median(kg)) * nc, 1)}
    full = out["settings"]["15x15x3"]
    out["search_over_replaced_route"] = {
        "host": round(full["enqueue_to_picks_host_ms"]["median_ms"] / out["replaced_route"]["host_ms_scaled"], 4),
        "kernels": round(full["register_maps_b_ms_per_launch"]["median_ms"] / out["replaced_route"]["kernels_ms_scaled"], 4)}
    B.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--shape", type=int, nargs=3, default=(128, 128, 24))
    ap.add_argument("--src-shape", type=int, nargs=3, default=(256, 256, 24))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--unique", type=int, default=8, help="phantom studies generated and repeated through the batch")
    ap.add_argument("--route-candidates", type=int, default=9, help="candidates the replaced route is measured on")
    ap.add_argument("--step", choices=("device",), help="run this one step in this process")
    ap.add_argument("--timeout", type=int, default=500, help="seconds per step")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "register_maps.json"))
    args = ap.parse_args()
    if args.rounds < 1 or args.unique < 1 or args.route_candidates < 1:
        sys.exit("--rounds, --unique and --route-candidates must be >= 1")
    if args.step:
        step_device(args)
        return
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "device", "--batch", str(args.batch),
           "--rounds", str(args.rounds), "--unique", str(args.unique), "--route-candidates", str(args.route_candidates),
           "--shape", *map(str, args.shape), "--src-shape", *map(str, args.src_shape)]
    try:
        p = subprocess.run(cmd, timeout=args.timeout, stdout=subprocess.PIPE, text=True)
    except subprocess.TimeoutExpired:
        sys.exit(f"step device: no end after {args.timeout} s")
    sys.stdout.write(p.stdout)
    if p.returncode != 0:
        sys.exit(f"step device ended with status {p.returncode}")
    with open(args.out, "w") as f:
        f.write(p.stdout.strip().splitlines()[-1] + "\n")


if __name__ == "__main__":
    main()
