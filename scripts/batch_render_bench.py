#!/usr/bin/env python3
"""The renderings of the device-resident bench batch, timed against the route they replace.

Inputs: bench.py's default batch (256 x 128x128x24, synth_batch base_seed 0, 64 unique studies,
vary=True), vox [1.5, 1.5, 10], the reference's 64-row parula table (tests/golden/parula.npy), no
proton.  Two steps, each a child process of its own under a time limit; the second starts only when
the first ended well:
  resident    one profiled Batch.run (N4 on), then --rounds rounds of Batch.overlay() and of
              Batch.montage() without and with a ci() before it: the overlay_b / montage_b kernel
              classes, and the host clock from the enqueue to the downloaded pixels.  Parity at this
              size is asserted for a handful of studies against _lib.overlay / _lib.montage on the
              downloaded arrays.
  host-route  what a caller does without them: Batch.download(n4=True) (+ download_ci("f64")), then
              _lib.overlay on the batch and _lib.montage per study, host clock.  The crops and the
              mask borders are computed before the clock starts (the class has them from its
              constructor).  Uses no call newer than download_ci, so the same file times an older build.
A study whose CI colour index passes the table's 64 rows (screenShot's IndexError) has no montage on
either route; both count them.  Prints one JSON line per step (profiles/batch_render.json holds them).
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
PARITY = (0, 1, 37, 63, 255)


def stats(ts, scale, unit):
    ts = np.asarray(ts) * scale
    return {"median_" + unit: round(float(np.median(ts)), 3), "min_" + unit: round(float(ts.min()), 3),
            "max_" + unit: round(float(ts.max()), 3), "n": int(ts.size)}


def parula():
    return np.load(os.path.join(REPO, "tests", "golden", "parula.npy"), allow_pickle=False)


def bench_batch(args):
    from vent_analysis_amd import _lib
    from vent_analysis_amd.synth import synth_batch
    R, C, Z = args.shape
    hp, mk = synth_batch(R, C, Z, args.batch, base_seed=0, unique=64, vary=True)
    B = _lib.Batch(R, C, Z, args.batch)
    B.upload(hp, mk)
    return B, hp, mk


def host_crop(mask):
    """cropToData(mask, border=5) as (r0, nr, c0, nc, s0, ns) (Vent_Analysis.py:430-456; index 0
    never counts as non-empty)."""
    out = []
    for ax, widen in ((0, 5), (1, 5), (2, 0)):
        on = np.flatnonzero(mask.any(axis=tuple(a for a in range(3) if a != ax)))
        on = on[on > 0]
        lo, hi = max(int(on[0]) - widen, 0), min(int(on[-1]) + widen + 1, mask.shape[ax])
        out += [lo, hi - lo]
    return tuple(out)


def step_resident(args):
    from vent_analysis_amd import _lib
    B, hp, mk = bench_batch(args)
    pal = parula()
    nb = args.batch
    B.run(B.options(do_n4=True, vox=VOX, profile=True))
    B.sync()

    # parity at the timed size
    n4, d, _, _, _ = B.download(n4=True)
    ov = B.overlay()
    parity = [q for q in PARITY if q < nb]
    for q in parity:
        assert np.array_equal(ov[q], _lib.overlay(n4[q], d[q])), q
    crop, off, lstatus = B.montage_layout()
    assert not lstatus.any()
    for q in parity:
        assert tuple(crop[q]) == host_crop(mk[q]), q
    borders = {q: _lib.border(mk[q])[0] for q in parity}
    zero = np.zeros(hp.shape[1:], np.float32)

    def montage_parity(ci):
        imgs, status = B.montage(pal)
        for q in parity:
            try:
                ref = _lib.montage(zero, hp[q], n4[q], borders[q], d[q], None if ci is None else ci[q], pal,
                                   crop[q])
            except IndexError:
                assert status[q] == _lib.VH_ERR_INDEX, q
                continue
            assert status[q] == _lib.VH_OK and np.array_equal(imgs[q], ref), q
        return int((status == _lib.VH_ERR_INDEX).sum())

    assert montage_parity(None) == 0
    B.ci(VOX)
    n_index = montage_parity(B.download_ci("f64")[0])
    del ov, n4, d

    def rounds(call, cls):
        call()   # warm-up (and the first call's allocations)
        kern, host, by = [], [], 0.0
        for _ in range(args.rounds):
            B.sync()
            B.reset_timers()
            t0 = time.perf_counter()
            call()
            host.append(time.perf_counter() - t0)
            ms, n, by = B.kernel_time(cls)
            assert n == 1, (cls, n)
            kern.append(ms)
        return stats(kern, 1e3, "us"), stats(host, 1e3, "ms"), by

    ok, oh, oby = rounds(B.overlay, "overlay_b")
    B.select_defect("mean", 1)   # the run's own maps again; the CI panel is blank from here
    mk0, mh0, mby0 = rounds(lambda: B.montage(pal), "montage_b")
    B.ci(VOX)
    B.sync()
    mk1, mh1, mby1 = rounds(lambda: B.montage(pal), "montage_b")
    B.close()
    print(json.dumps({
        "what": "batch_render", "step": "resident", "shape": list(args.shape), "batch": nb,
        "rounds": args.rounds, "parity_studies": parity, "montage_bytes": int(off[-1]),
        "overlay_bytes": 3 * int(np.prod(hp.shape)), "studies_with_index_error_under_ci": n_index,
        "overlay_b_us": ok, "overlay_b_bytes_per_launch": oby, "overlay_host_ms": oh,
        "montage_b_us": mk0, "montage_b_bytes_per_launch": mby0, "montage_host_ms": mh0,
        "montage_b_with_ci_us": mk1, "montage_b_with_ci_bytes_per_launch": mby1,
        "montage_with_ci_host_ms": mh1,
        "host_clock": "enqueue to downloaded pixels, layout included (cached after the first call)"}))


def step_host_route(args):
    from vent_analysis_amd import _lib
    B, hp, mk = bench_batch(args)
    pal = parula()
    nb = args.batch
    B.run(B.options(do_n4=True, vox=VOX))
    B.ci(VOX)
    B.sync()
    crops = [host_crop(mk[q]) for q in range(nb)]          # not timed: the class has both from
    borders = _lib.border(mk)                               # its constructor
    zero = np.zeros(hp.shape[1:], np.float32)

    def overlay_route():
        n4, d, _, _, _ = B.download(n4=True)
        return _lib.overlay(n4, d)

    def montage_route(with_ci):
        n4, d, _, _, _ = B.download(n4=True)
        ci = B.download_ci("f64")[0] if with_ci else None
        failed = 0
        for q in range(nb):
            try:
                _lib.montage(zero, hp[q], n4[q], borders[q], d[q], None if ci is None else ci[q], pal, crops[q])
            except IndexError:
                failed += 1
        return failed

    def rounds(call):
        call()
        ts = []
        for _ in range(args.host_rounds):
            t0 = time.perf_counter()
            call()
            ts.append(time.perf_counter() - t0)
        return stats(ts, 1e3, "ms")

    o = rounds(overlay_route)
    m0 = rounds(lambda: montage_route(False))
    n_index = montage_route(True)
    m1 = rounds(lambda: montage_route(True))
    B.close()
    print(json.dumps({"what": "batch_render", "step": "host-route", "shape": list(args.shape), "batch": nb,
                      "rounds": args.host_rounds, "studies_with_index_error_under_ci": n_index,
                      "overlay_host_ms": o, "montage_host_ms": m0, "montage_with_ci_host_ms": m1,
                      "not_timed": "cropToData and calculateBorder of the masks"}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--shape", type=int, nargs=3, default=(128, 128, 24))
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--host-rounds", type=int, default=3, help="rounds of each host route")
    ap.add_argument("--step", choices=("resident", "host-route"), help="run this one step in this process")
    ap.add_argument("--timeout", type=int, default=400, help="seconds per step")
    args = ap.parse_args()
    if args.rounds < 1 or args.host_rounds < 1:
        sys.exit("--rounds and --host-rounds must be >= 1")
    if args.step:
        {"resident": step_resident, "host-route": step_host_route}[args.step](args)
        return
    for step in ("resident", "host-route"):   # chained: a failed or hung step ends the script
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
