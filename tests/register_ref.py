"""The numpy reference of the proton-to-xenon registration (include/vent_hip.h, "the proton registered
to the xenon image"): the 32-level codes, the joint histogram of a shift by slicing and np.bincount, the
mutual information in float64, the pick and the shift; and the seeded phantom the host and GPU tests
share.  Every count is an integer; only mi is floating point."""
import functools

import numpy as np

LEVELS = 32
INVALID = 255

# (shape, search window, the planted shift of studies 0..2): the GPU test's cases
CASES = [
    ((41, 37, 9), (4, 4, 2), [(3, -2, 1), (-4, 1, -1), (0, 3, -2)]),      # V is no multiple of 16
    ((9, 131, 32), (2, 8, 1), [(1, -6, 1), (-2, 8, 0), (2, 3, -1)]),
    ((33, 40, 33), (2, 3, 2), [(2, -1, 1), (-1, 3, -2), (0, -3, 2)]),
    ((64, 64, 24), (4, 4, 1), [(3, -2, 1), (-4, 1, -1), (2, -1, 1)]),
    ((128, 128, 24), (2, 2, 1), [(2, -1, 1), (-2, 1, -1)]),               # studies 0 and 1 only
    ((12, 10, 1), (1, 1, 0), [(1, -1, 0), (-1, 1, 0), (0, 1, 0)]),
]
PLANTED = {shape: planted for shape, _, planted in CASES}


# ---- codes, joint histogram, score, pick, shift -------------------------------------------------------
def image_max(x):
    """The maximum over F (finite and >= 0) as float32; +0.0 when F is empty."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        f = x[np.isfinite(x) & (x >= 0)]
    return np.float32(abs(f.max())) if f.size else np.float32(0)


def codes(x):
    """One study -> uint8 codes of its shape, 255 where the voxel is invalid; None when the maximum is
    not > 0 (the study is unregistrable)."""
    x = np.asarray(x, np.float32)
    m = image_max(x)
    if not m > 0:
        return None
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        valid = np.isfinite(x) & (x >= 0)
        scale = np.float32(256.0) / m
        prod = (np.where(valid, x, np.float32(0)) * scale).astype(np.float32)
        small = prod < np.float32(255.0)            # (NaN -- an infinite scale times zero -- is not)
        bins = np.where(small, np.where(small, prod, 0).astype(np.int64), 255)
    return np.where(valid, bins >> 3, INVALID).astype(np.uint8)


def _windows(n, d):
    """The slices of v and of v + d along an axis of n voxels, both inside it."""
    return slice(max(0, -d), n - max(0, d)), slice(max(0, d), n - max(0, -d))


def joint(cp, cx, s):
    """J_s[a][b] uint32 [32][32]: a the code of P(v + s), b the code of X(v), over the v for which both
    voxels are inside the volume and valid."""
    v, vs = zip(*(_windows(n, d) for n, d in zip(cx.shape, s)))
    a = cp[vs].astype(np.int64).reshape(-1)
    b = cx[v].astype(np.int64).reshape(-1)
    ok = (a != INVALID) & (b != INVALID)
    return np.bincount(a[ok] * LEVELS + b[ok], minlength=LEVELS * LEVELS).astype(np.uint32).reshape(LEVELS, LEVELS)


def mi(J):
    """(1 / n) sum over J > 0 of J log((J n) / (Ja Jb)) in float64; 0.0 for an empty histogram."""
    J = np.asarray(J).astype(np.int64)
    n = int(J.sum())
    if n == 0:
        return 0.0
    ja, jb = J.sum(axis=1), J.sum(axis=0)
    a, b = np.nonzero(J)
    j = J[a, b].astype(np.float64)
    num = j * np.float64(n)
    den = ja[a].astype(np.float64) * jb[b].astype(np.float64)
    return float(np.sum(j * np.log(num / den)) / np.float64(n))


def shifts(search):
    """Every (dr, dc, dz) of the window in index order: dz slowest, then dr, then dc."""
    Sr, Sc, Sz = (int(v) for v in search)
    return [(dr, dc, dz) for dz in range(-Sz, Sz + 1) for dr in range(-Sr, Sr + 1) for dc in range(-Sc, Sc + 1)]


def pick(score, search):
    """The best shift of one study's scores: the largest, then the smallest L1 norm, then the lowest
    index; a NaN never wins, and nothing but NaN gives (0, 0, 0)."""
    best, key = (0, 0, 0), None
    for i, (s, v) in enumerate(zip(shifts(search), np.asarray(score, np.float64).reshape(-1))):
        if np.isnan(v):
            continue
        k = (-float(v), sum(abs(d) for d in s), i)
        if key is None or k < key:
            best, key = s, k
    return best


def gap(score):
    """The best score minus the second best (inf with a single shift)."""
    v = np.sort(np.asarray(score, np.float64).reshape(-1))
    return float(v[-1] - v[-2]) if v.size > 1 else float("inf")


def shift_image(a, s):
    """A'(v) = A(v + s) where v + s is inside the volume, 0 elsewhere; the last three axes are R, C, Z."""
    a = np.asarray(a)
    out = np.zeros_like(a)
    v, vs = zip(*(_windows(n, int(d)) for n, d in zip(a.shape[-3:], s)))
    out[(Ellipsis,) + tuple(v)] = a[(Ellipsis,) + tuple(vs)]
    return out


# ---- the phantom -------------------------------------------------------------------------------------
def _anatomy(shape, s):
    """(body, lungs, vent) on the grid displaced by s: body and lungs bool, vent the xenon's texture."""
    R, C, Z = shape
    r, c, z = np.meshgrid(np.arange(R) + s[0], np.arange(C) + s[1], np.arange(Z) + s[2], indexing="ij")
    u, w = (r - (R - 1) / 2) / R, (c - (C - 1) / 2) / C
    t = (z - (Z - 1) / 2) / max(Z, 2)                       # -0.5 .. 0.5 through the slices
    grow = 1.0 - 1.6 * t * t + 0.3 * t                      # the lungs vary with the slice
    body = (u / 0.38) ** 2 + (w / 0.34) ** 2 < 1.0
    left = (u / (0.24 * grow)) ** 2 + ((w + 0.16) / (0.10 * grow)) ** 2 < 1.0
    right = ((u - 0.03) / (0.21 * grow)) ** 2 + ((w - 0.17) / (0.11 * grow)) ** 2 < 1.0
    vent = 0.75 + 0.25 * np.sin(9.0 * u + 3.0 * t) * np.cos(11.0 * w - 2.0 * t)
    return body, (left | right) & body, vent


def _rician(rng, signal, sigma):
    return np.sqrt((signal + rng.normal(0, sigma, signal.shape)) ** 2 + rng.normal(0, sigma, signal.shape) ** 2)


def study(shape, planted, kind, seed):
    """(proton, xenon) float32 of one study.  The xenon lies on the grid; the proton is the same anatomy
    displaced so that proton(v + planted) matches xenon(v).  kind 0: Rician-like noise everywhere; 1: the
    background of both images exactly 0; 2: as 0, salted with NaN, +-inf and negative voxels."""
    rng = np.random.default_rng(seed)
    R, C, Z = shape
    body_x, lungs_x, vent = _anatomy(shape, (0, 0, 0))
    body_p, lungs_p, _ = _anatomy(shape, tuple(-d for d in planted))
    r = np.arange(R)[:, None, None] / R
    quiet = 0.25 if R * C * Z < 1000 else 1.0          # (a few hundred voxels carry the shift only at low noise)
    xenon = _rician(rng, np.where(lungs_x, 80.0 * vent, 0.0), 3.0 * quiet)
    proton = _rician(rng, np.where(body_p, np.where(lungs_p, 12.0, 100.0 + 30.0 * r), 0.0), 4.0 * quiet)
    if kind == 1:
        xenon = np.where(lungs_x, xenon, 0.0)
        proton = np.where(body_p, proton, 0.0)
    if kind == 2:
        for img in (proton, xenon):
            at = rng.random(shape)
            img[at < 0.004] = np.nan
            img[(at >= 0.004) & (at < 0.006)] = np.inf
            img[(at >= 0.006) & (at < 0.008)] = -np.inf
            img[(at >= 0.008) & (at < 0.014)] *= -1.0
    return proton.astype(np.float32), xenon.astype(np.float32)


@functools.lru_cache(maxsize=None)
def batch(shape):
    """(proton, xenon) float32 [4][R][C][Z], read-only: studies 0..2 of kinds 0..2 with the planted shifts
    of PLANTED (zero where the table has none), study 3 a constant proton."""
    planted = list(PLANTED.get(shape, [])) + [(0, 0, 0)] * 4
    ps, xs = [], []
    for q in range(4):
        p, x = study(shape, planted[q], min(q, 2) if q < 3 else 0, 1000 * q + sum(shape))
        if q == 3:
            p = np.full(shape, 7.5, np.float32)
        ps.append(p)
        xs.append(x)
    P, X = np.stack(ps), np.stack(xs)
    P.setflags(write=False)
    X.setflags(write=False)
    return P, X


@functools.lru_cache(maxsize=None)
def reference(shape, search, n=4):
    """(hist uint32 [n][ns][32][32], score float64 [n][ns], best [n] of tuples, gap [n]) of the first n
    studies of batch(shape), read-only."""
    P, X = batch(shape)
    return reference_of(P[:n], X[:n], search)


def reference_of(P, X, search):
    sh = shifts(search)
    n = len(P)
    hist = np.zeros((n, len(sh), LEVELS, LEVELS), np.uint32)
    score = np.zeros((n, len(sh)), np.float64)
    best, gaps = [], []
    for q in range(n):
        cp, cx = codes(P[q]), codes(X[q])
        if cp is None or cx is None:
            score[q] = np.nan
            best.append((0, 0, 0))
            gaps.append(float("nan"))
            continue
        for i, s in enumerate(sh):
            hist[q, i] = joint(cp, cx, s)
            score[q, i] = mi(hist[q, i])
        best.append(pick(score[q], search))
        gaps.append(gap(score[q]))
    hist.setflags(write=False)
    score.setflags(write=False)
    return hist, score, best, gaps
