#!/usr/bin/env python3
"""Cluster index of the device-resident bench batch: the routes to it, timed against each other.

Inputs: bench.py's default batch (256 x 128x128x24, synth_batch base_seed 0, 64 unique studies,
vary=True), vox [1.5, 1.5, 10], Rmax 50.  One Batch.run, one warm-up of each route, then --rounds
rounds alternating the routes in this process, each timed by the host clock around work that ends in
a synchronise:
  a  Batch.download() of the defect maps, then _lib.ci(defect, table, 1.5, shell=False)
  b  Batch.ci() + download_ci(maps=None)
  c  Batch.ci() + download_ci(maps="shell")
  d  route b under VH_CI_FORM=1
A second pass with profiling on records the kernel classes ci_walk (VH_CI_FORM=1) and ci_walk_b
(VH_CI_FORM=2) on the same resident batch, and again on batches of --small studies.  Shells, scalars
and status of forms 1 and 2 are asserted equal on every study, and four studies against the CPU
oracle.  Prints one JSON line (profiles/ci_batch.json).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

VOX = (1.5, 1.5, 10.0)
RMAX = 50


def stats(ts):
    ts = np.asarray(ts) * 1e3
    return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(float(ts.min()), 3),
            "max_ms": round(float(ts.max()), 3), "n": int(ts.size)}


def with_form(form, fn):
    old = os.environ.get("VH_CI_FORM")
    if form is None:
        os.environ.pop("VH_CI_FORM", None)
    else:
        os.environ["VH_CI_FORM"] = str(form)
    try:
        return fn()
    finally:
        if old is None:
            os.environ.pop("VH_CI_FORM", None)
        else:
            os.environ["VH_CI_FORM"] = old


def kernel_times(B, rounds):
    """Per-launch times (us) of the two walk kernels on B's resident maps, alternating the forms."""
    out = {}
    per = {1: [], 2: []}
    for _ in range(rounds):
        for form, name in ((1, "ci_walk"), (2, "ci_walk_b")):
            B.reset_timers()
            with_form(form, lambda: B.ci(VOX, RMAX))
            B.sync()
            ms, n, _ = B.kernel_time(name)
            assert n == 1, (name, n)
            per[form].append(ms * 1e3)
    for form, name in ((1, "ci_walk"), (2, "ci_walk_b")):
        t = np.asarray(per[form])
        out[name] = {"median_us": round(float(np.median(t)), 2), "min_us": round(float(t.min()), 2),
                     "max_us": round(float(t.max()), 2), "n": int(t.size)}
    a, b = out["ci_walk"], out["ci_walk_b"]
    out["ranges_overlap"] = not (b["max_us"] < a["min_us"] or a["max_us"] < b["min_us"])
    out["batch_form_faster"] = b["max_us"] < a["min_us"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--small", type=int, nargs="+", default=(4, 16), help="studies of the few-study batches")
    ap.add_argument("--shape", type=int, nargs=3, default=(128, 128, 24))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--no-n4", action="store_true", help="N4 := identity in the one Batch.run")
    args = ap.parse_args()
    if args.rounds < 1:
        sys.exit("--rounds must be >= 1")

    from oracle import native, vdp_oracle as O
    from vent_analysis_amd import _lib
    from vent_analysis_amd.sphere import compact_table_for
    from vent_analysis_amd.synth import synth_batch

    R, C, Z = args.shape
    nb = args.batch
    hp, mk = synth_batch(R, C, Z, nb, base_seed=0, unique=64, vary=True)
    table = compact_table_for(VOX, RMAX, (R, C, Z))
    B = _lib.Batch(R, C, Z, nb)
    B.upload(hp, mk)
    B.run(B.options(do_n4=not args.no_n4, vox=VOX, do_cohort=True))
    B.sync()

    def route_a():
        _, d, _, _, _ = B.download()
        return _lib.ci(d, table, 1.5, shell=False)

    def route_b():
        B.ci(VOX, RMAX)
        return B.download_ci(maps=None)

    def route_c():
        B.ci(VOX, RMAX)
        return B.download_ci(maps="shell")

    routes = {"a": route_a, "b": lambda: with_form(None, route_b), "c": lambda: with_form(None, route_c),
              "d": lambda: with_form(1, route_b)}
    for fn in routes.values():   # one warm-up each (tables, workspaces, pinned buffers)
        fn()
    ts = {k: [] for k in routes}
    for _ in range(args.rounds):
        for k, fn in routes.items():
            t0 = time.perf_counter()
            fn()
            ts[k].append(time.perf_counter() - t0)

    # parity at the timed size: forms 1 and 2 on every study, four studies against the CPU oracle
    f1 = with_form(1, route_c)
    f2 = with_form(2, route_c)
    for x, y in zip(f1, f2):
        assert np.array_equal(x, y, equal_nan=True), "forms 1 and 2 differ"
    _, d, _, _, _ = B.download()
    checked = []
    for q in sorted({0, nb // 3, (2 * nb) // 3, nb - 1}):
        try:
            ref, shell = native.ci(d[q], table, VOX)
            assert f2[2][q] == _lib.VH_OK and np.array_equal(f2[0][q], shell.astype(np.int16))
            assert f2[1][q] == O.ci_scalar(ref[d[q] != 0])
            assert np.array_equal(_lib.ci_expand(f2[0][q], table.radii, 1.5), ref)
        except ValueError:
            assert f2[2][q] == _lib.VH_ERR_MAXRADIUS
        checked.append(q)

    # kernel classes, profiling on, same resident maps
    B.run(B.options(do_n4=False, vox=VOX, profile=True))   # switches the batch's timers on
    B.upload_defect(d)                                     # the timed maps again (the N4 run's)
    B.sync()
    with_form(1, lambda: B.ci(VOX, RMAX))
    with_form(2, lambda: B.ci(VOX, RMAX))
    kt = kernel_times(B, args.rounds)
    defects = [int(x) for x in (d != 0).reshape(nb, -1).sum(axis=1)]
    status = [int(x) for x in f2[2]]
    B.close()

    small = {}
    for ns in args.small:
        Bs = _lib.Batch(R, C, Z, ns)
        Bs.upload(hp[:ns], mk[:ns])
        Bs.run(Bs.options(do_n4=False, vox=VOX, profile=True))
        Bs.upload_defect(d[:ns])
        Bs.sync()
        with_form(1, lambda: Bs.ci(VOX, RMAX))
        with_form(2, lambda: Bs.ci(VOX, RMAX))
        small["batch_%d" % ns] = kernel_times(Bs, args.rounds)
        s1 = with_form(1, lambda: (Bs.ci(VOX, RMAX), Bs.download_ci())[1])
        s2 = with_form(2, lambda: (Bs.ci(VOX, RMAX), Bs.download_ci())[1])
        for x, y in zip(s1, s2):
            assert np.array_equal(x, y, equal_nan=True), "forms 1 and 2 differ on a small batch"
        for x, y in zip(s2, f2):
            assert np.array_equal(x, y[:ns], equal_nan=True), "a small batch differs from the large one"
        Bs.close()

    out = {"what": "ci_batch", "shape": [R, C, Z], "batch": nb, "vox": list(VOX), "Rmax": RMAX,
           "n4_in_the_run": not args.no_n4, "rounds": args.rounds,
           "table": {"rows": table.rows, "shells": int(table.bounds.shape[0])},
           "defect_voxels": {"total": int(sum(defects)), "min": min(defects), "max": max(defects)},
           "status_counts": {str(s): status.count(s) for s in sorted(set(status))},
           "routes_host_clock": {
               "a_download_then_lib_ci_f64": stats(ts["a"]),
               "b_batch_ci_scalars": stats(ts["b"]),
               "c_batch_ci_shell_map": stats(ts["c"]),
               "d_batch_ci_scalars_form1": stats(ts["d"])},
           "kernel_us": {"batch_%d" % nb: kt, **small},
           "parity": {"forms_equal_studies": nb, "oracle_studies": checked},
           "env": {k: os.environ.get(k) for k in ("VH_CI_FORM", "VH_CI_B_ROWS", "VH_CI_B_G")}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
