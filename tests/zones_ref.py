"""Inputs and the numpy reference of the regional-analysis tests (test_zones_host.py,
test_gpu_zones.py): the zone rule of include/vent_hip.h -- bounds, parts of an axis by extent or by
count, the lateral split, the zone of a voxel -- in Python integers, and per zone the counts, the
histogram and the fixed-point sum by the distribution's rule (distribution_ref).  Every value is an
integer.  Not a test module."""
import functools

import numpy as np

import distribution_ref as DR

F32 = np.float32
COLS = 8
FX = F32(16777216.0)                     # 2^24: the fixed-point scale of the sum
EXTENT, COUNT = 0, 1
VOX = DR.VOX
# the prototype's shapes, then more slices than a workgroup has threads and a long row
SHAPES = [(7, 5, 3), (12, 9, 1), (33, 20, 5), (41, 37, 9), (64, 64, 24), (130, 19, 2), (12, 10, 300), (4, 62, 1000)]
N_STUDIES = 7


# ---- the rule ------------------------------------------------------------------------------------
def bounds(P):
    """(lo, hi): the first and the last index with P > 0; (0, -1) for an all-zero profile."""
    nz = [i for i, x in enumerate(P) if int(x) > 0]
    return (nz[0], nz[-1]) if nz else (0, -1)


def axis_parts(P, p, by):
    """uint8 [n]: the part of every index of an axis with profile P, in Python integers (floored //)."""
    P = [int(x) for x in P]
    lo, hi = bounds(P)
    w, total = hi - lo + 1, sum(P)
    if by in (EXTENT, "extent"):
        part = [0 if w <= 0 else min(p - 1, max(0, ((i - lo) * p) // w)) for i in range(len(P))]
    else:
        part, cum = [], 0
        for x in P:
            part.append(0 if total == 0 else min(p - 1, (cum * p) // total))
            cum += x
    return np.array(part, np.uint8)


def split(P):
    """The lateral split column: the smallest P among lo + w // 4 .. hi - w // 4, ties to the smallest
    column; 0 for an all-zero profile."""
    P = [int(x) for x in P]
    lo, hi = bounds(P)
    if hi < lo:
        return 0
    q = (hi - lo + 1) // 4
    return min(range(lo + q, hi - q + 1), key=lambda c: (P[c], c))


def profiles(mask):
    on = np.asarray(mask) != 0
    return on.sum(axis=(1, 2)), on.sum(axis=(0, 2)), on.sum(axis=(0, 1))


def n_zones(parts, lateral):
    return int(parts[0]) * (2 if lateral else int(parts[1])) * int(parts[2])


def geometry(mask, lateral):
    """int32 [8]: lo_r, hi_r, lo_c, hi_c, lo_z, hi_z, s (-1 without lateral), 0."""
    Pr, Pc, Pz = profiles(mask)
    return np.array([*bounds(Pr), *bounds(Pc), *bounds(Pz), split(Pc) if lateral else -1, 0], np.int32)


def zone_map(mask, parts, lateral, by):
    """uint8 [R][C][Z]: 1 + (part_r nc + col) pz + part_z on the mask, 0 off it."""
    on = np.asarray(mask) != 0
    Pr, Pc, Pz = profiles(mask)
    pr = axis_parts(Pr, parts[0], by).astype(np.int64)
    pz = axis_parts(Pz, parts[2], by).astype(np.int64)
    if lateral:
        assert parts[1] == 1
        col, nc = (np.arange(on.shape[1]) >= split(Pc)).astype(np.int64), 2
    else:
        col, nc = axis_parts(Pc, parts[1], by).astype(np.int64), int(parts[1])
    zone = 1 + (pr[:, None, None] * nc + col[None, :, None]) * int(parts[2]) + pz[None, None, :]
    return np.where(on, zone, 0).astype(np.uint8)


def label_zones(mask, labels, K):
    """The caller's zones: a byte 1..K on the mask stays, any other byte on the mask is 0, like every
    byte off it."""
    lab = np.asarray(labels)
    return np.where((np.asarray(mask) != 0) & (lab >= 1) & (lab <= K), lab, 0).astype(np.uint8)


def zone_counts(N4, mask, defect, lb, zmap, K, norm, bins, hi):
    """dict(counts int64 [K + 1][8], hist uint32 [K + 1][bins], stats int64 [K + 1][4]) of one study over
    mask != 0: the distribution's histogram rule per zone, n_in / n_below / n_over and the sum of
    int64(float32(nv * 2^24)) over the in-range voxels."""
    counts = np.zeros((K + 1, COLS), np.int64)
    hist = np.zeros((K + 1, bins), np.uint32)
    stats = np.zeros((K + 1, 4), np.int64)
    on = np.asarray(mask) != 0
    m, p99 = DR.anchors(N4, mask)
    if m is None:
        return dict(counts=counts, hist=hist, stats=stats)
    d = F32(m if norm in ("mean", 0) else p99)
    with np.errstate(divide="ignore", invalid="ignore"):
        nv = (np.asarray(N4, dtype=F32)[on] / d).astype(F32)
        inside = (nv >= 0) & (nv < F32(hi))
        scale = F32(F32(bins) / F32(hi))
        bi = np.minimum(bins - 1, (nv[inside] * scale).astype(F32).astype(np.int64))
        fx = (nv[inside] * FX).astype(F32).astype(np.int64)
    z = np.asarray(zmap)[on].astype(np.int64)
    df = np.asarray(defect)[on] != 0
    cl = np.asarray(lb)[on]
    assert z.max(initial=0) <= K
    for k in range(K + 1):
        sel = z == k
        counts[k] = [sel.sum(), (sel & df).sum()] + [(sel & (cl == c)).sum() for c in range(1, 7)]
        hist[k] = np.bincount(bi[sel[inside]], minlength=bins)
        below = int((sel & (nv < 0)).sum())
        n_in = int((sel & inside).sum())
        stats[k] = [n_in, below, int(sel.sum()) - n_in - below, fx[sel[inside]].sum()]
    return dict(counts=counts, hist=hist, stats=stats)


# ---- the inputs ----------------------------------------------------------------------------------
def lungs(shape, bridge=False):
    """Two ellipses with a gap of whole columns between them, tapering towards the end slices; with
    ``bridge`` one row joins them across the gap."""
    R, C, Z = shape
    g0 = max(1, int(C * 0.45))
    g1 = max(g0 + 1, int(np.ceil(C * 0.55)))          # the gap: columns g0 .. g1 - 1
    r = np.arange(R)[:, None, None] + 0.5
    c = np.arange(C)[None, :, None] + 0.5
    z = np.arange(Z)[None, None, :]
    taper = 1 - 0.3 * np.abs(z - (Z - 1) / 2) / Z

    def ellipse(c0, c1):
        return ((c - (c0 + c1) / 2) / ((c1 - c0) / 2 * taper)) ** 2 + ((r - R / 2) / (0.45 * R * taper)) ** 2 <= 1
    m = ellipse(0, g0) | ellipse(g1, C)
    if bridge:
        m[R // 2, g0 - 1:g1 + 1, :] = True
    return m.astype(np.uint8)


def gap(shape):
    C = shape[1]
    g0 = max(1, int(C * 0.45))
    return g0, max(g0 + 1, int(np.ceil(C * 0.55)))


def studies(shape):
    """Seven studies.  Masks: two lungs with a clear gap, two lungs with a bridge, empty, all ones, a
    single column (w_c = 1: side 0 is empty), the gap again, the bridge again.  Values: the two fields
    of distribution_ref; study 5 has a few masked values negated (n_below), study 6 every masked value
    0 (d = 0: NaN fills n_over)."""
    X1, _ = DR.D.field(shape, 1)
    X2, _ = DR.D.field(shape, 2)
    one = np.zeros(shape, np.uint8)
    one[:, shape[1] // 2, :] = 1
    mk = np.stack([lungs(shape), lungs(shape, True), np.zeros(shape, np.uint8), np.ones(shape, np.uint8), one,
                   lungs(shape), lungs(shape, True)])
    neg = X2.copy()
    idx = np.flatnonzero(mk[5])
    pick = idx[np.random.default_rng(5).choice(idx.size, size=min(7, idx.size), replace=False)]
    neg.reshape(-1)[pick] *= F32(-0.5)
    zero = np.where(mk[6] != 0, F32(0), X1).astype(F32)
    hp = np.stack([X1, X2, X1, X2, X1, neg, zero])
    assert hp.shape[0] == N_STUDIES
    return hp, mk


@functools.lru_cache(maxsize=None)
def batch_inputs(shape):
    """(hp, mask) of studies(shape), computed once and read-only."""
    hp, mk = studies(shape)
    hp.setflags(write=False)
    mk.setflags(write=False)
    return hp, mk


@functools.lru_cache(maxsize=None)
def batch_maps(shape):
    """(defect, lb) of batch_inputs(shape) after a plain run with N4 = identity, in numpy."""
    hp, mk = batch_inputs(shape)
    defect = np.stack([DR.run_defect(x, m) for x, m in zip(hp, mk)]).astype(np.uint8)
    lb = np.stack([DR.lb_volume(x, m) for x, m in zip(hp, mk)]).astype(np.uint8)
    defect.setflags(write=False)
    lb.setflags(write=False)
    return defect, lb


def reference(N4, mask, defect, lb, parts=(3, 1, 1), lateral=True, by=EXTENT, labels=None, K=None, norm="mean",
              bins=100, hi=1.5):
    """One study's whole result: map, counts, hist, stats, geom."""
    if labels is None:
        K = n_zones(parts, lateral)
        zmap = zone_map(mask, parts, lateral, by)
    else:
        zmap = label_zones(mask, labels, K)
    out = zone_counts(N4, mask, defect, lb, zmap, K, norm, bins, hi)
    out.update(map=zmap, geom=geometry(mask, lateral and labels is None))
    return out


def assert_equal(got, refs, keys=("map", "counts", "hist", "stats", "geom")):
    """Batch.download_zones's dict against the per-study references, exactly."""
    for q, r in enumerate(refs):
        for k in keys:
            assert got[k][q].dtype == r[k].dtype, (k, got[k].dtype, r[k].dtype)
            assert got[k][q].shape == r[k].shape, (q, k, got[k][q].shape, r[k].shape)
            assert np.array_equal(got[k][q], r[k]), (q, k, got[k][q], r[k])
