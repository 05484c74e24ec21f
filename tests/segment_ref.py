"""The numpy reference of the proton segmentation (include/vent_hip.h, "the lungs from the proton
image"): the statistics, the Otsu cut in double and in exact rationals, the threshold, the
border-seeded flood fill by directional sweeps and the opening; and the seeded inputs the host and GPU
tests share.  No scipy here: the host test compares this file against scipy.ndimage."""
import functools
from fractions import Fraction

import numpy as np

import mask_edit_ref as M

SHAPES = [(41, 37, 9), (64, 64, 24), (33, 40, 33), (9, 131, 32)]
BIG = (512, 512, 2)                       # the largest plane the kernel takes: studies 0 and 1 only
RADII = [(0, 0, 0, 0), (1, 2, 0, 5), (3, 0, 3, 0)]   # one open_radius per study of batch_proton
THRESH = (40.0, 0.5, 4.0, 50.0)           # the explicit threshold of each study
ZCS = (1, 2, 4, 8, 16, 32)
LDS_MAX = 156 * 1024


def zc_fits(shape, zc):
    """Both bit sets of the plane fit the kernel's LDS budget at ``zc`` slices per field."""
    R, C, _ = shape
    wpr = (C * zc + 31) // 32
    return 2 * 4 * R * (wpr | 1) <= LDS_MAX


# ---- statistics, Otsu, threshold -----------------------------------------------------------------
def stats(x):
    """One study -> (pmax float32, hist uint32 [256])."""
    x = np.asarray(x, np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        f = x[np.isfinite(x) & (x >= 0)]
    hist = np.zeros(256, np.uint32)
    pmax = np.float32(f.max()) if f.size else np.float32(0)
    if not pmax > 0:
        return np.float32(abs(pmax)), hist
    scale = np.float32(256.0) / pmax
    prod = (f * scale).astype(np.float32)
    bins = np.minimum(255, prod.astype(np.int64))
    hist += np.bincount(bins, minlength=256).astype(np.uint32)
    return pmax, hist


def otsu_double(h):
    """The cut as the library evaluates it: Python floats are doubles, one rounding per operation.
    None when fewer than two bins are occupied."""
    h = [int(v) for v in h]
    if sum(v != 0 for v in h) < 2:
        return None
    N, S = float(sum(h)), float(sum(i * v for i, v in enumerate(h)))
    n0i = s0i = 0
    best, at = -1.0, None
    for k in range(len(h) - 1):
        n0i += h[k]
        s0i += k * h[k]
        if n0i == 0 or n0i == sum(h):
            continue
        n0, s0 = float(n0i), float(s0i)
        d = S * n0 - N * s0
        v = d * d / (n0 * (N - n0))
        if v > best:
            best, at = v, k
    return at


def otsu_values(h):
    """{k: the criterion as an exact Fraction} over the cuts that are not skipped."""
    h = [int(v) for v in h]
    N, S = sum(h), sum(i * v for i, v in enumerate(h))
    out, n0, s0 = {}, 0, 0
    for k in range(len(h) - 1):
        n0 += h[k]
        s0 += k * h[k]
        if n0 == 0 or n0 == N:
            continue
        d = S * n0 - N * s0
        out[k] = Fraction(d * d, n0 * (N - n0))
    return out


def otsu_exact(h):
    """The lowest k of the exact maximum; None when fewer than two bins are occupied."""
    if sum(int(v) != 0 for v in h) < 2:
        return None
    vals = otsu_values(h)
    best = max(vals.values())
    return min(k for k, v in vals.items() if v == best)


def otsu_margin(h):
    """(best - second best distinct value) / best as a float; None with one distinct value only."""
    vals = sorted(set(otsu_values(h).values()))
    if len(vals) < 2:
        return None
    return float((vals[-1] - vals[-2]) / vals[-1])


def threshold(x):
    """One study -> float32 threshold, NaN where it is undefined."""
    pmax, hist = stats(x)
    k = otsu_exact(hist) if pmax > 0 else None
    if k is None:
        return np.float32(np.nan)
    return np.float32(k + 1) * (pmax / np.float32(256.0))


# ---- the fill ------------------------------------------------------------------------------------
def _sweep_round(dark, reach):
    """One round of the four directional sweeps, in place, every slice at once; True if it changed."""
    before = reach.copy()
    R, C = dark.shape[:2]
    for c in range(1, C):
        reach[:, c] |= dark[:, c] & reach[:, c - 1]
    for c in range(C - 2, -1, -1):
        reach[:, c] |= dark[:, c] & reach[:, c + 1]
    for r in range(1, R):
        reach[r] |= dark[r] & reach[r - 1]
    for r in range(R - 2, -1, -1):
        reach[r] |= dark[r] & reach[r + 1]
    return not np.array_equal(before, reach)


def flood(dark):
    """(reach, rounds): the dark pixels joined to a dark border pixel of their slice under
    4-connectivity, bool [R][C][Z] (or [R][C]), and the rounds that changed something."""
    dark = np.asarray(dark, bool)
    edge = np.zeros(dark.shape, bool)
    edge[0] = edge[-1] = True
    edge[:, 0] = edge[:, -1] = True
    reach = dark & edge
    rounds = 0
    while _sweep_round(dark, reach):
        rounds += 1
    return reach, rounds


def segment(x, t, open_radius=0):
    """One study, float32 [R][C][Z] -> uint8 0 / 1."""
    with np.errstate(invalid="ignore"):
        dark = np.asarray(x, np.float32) < np.float32(t)
    seg = dark & ~flood(dark)[0]
    if open_radius:
        seg = M.open_(seg, int(open_radius))
    return seg.astype(np.uint8)


def batch_segment(xs, ts, radii):
    return np.stack([segment(x, t, k) for x, t, k in zip(xs, ts, radii)])


# ---- the shared inputs ---------------------------------------------------------------------------
def _ellipse(R, C, r0, c0, a, b):
    rr, cc = np.mgrid[0:R, 0:C]
    return ((rr - r0) / max(a, 0.5)) ** 2 + ((cc - c0) / max(b, 0.5)) ** 2 <= 1.0


def maze_layout(L, S):
    """The maze of study 1 with its long axis along the rows, [L][S] bool dark, closed: a one-pixel
    serpentine corridor (runs on rows 2, 4, ... over columns 1 .. S - 2, joined at alternating ends),
    and below it a dark band open to the border that holds a one-pixel diagonal bright diamond.
    Returns (dark, runs, the wall pixel between the first two runs, a corridor pixel, the diamond's
    centre)."""
    dark = np.zeros((L, S), bool)
    rows = list(range(2, L - 13, 2))[:24]
    for i, r in enumerate(rows):
        dark[r, 1:S - 1] = True
        if i + 1 < len(rows):
            dark[r + 1, S - 2 if i % 2 == 0 else 1] = True
    dark[L - 10:, :] = True
    r0, c0 = L - 6, S // 2
    for k in range(-3, 4):
        w = 3 - abs(k)
        dark[r0 + k, c0 - w] = dark[r0 + k, c0 + w] = False
    return dark, len(rows), (3, S // 2), (rows[1], S // 2), (r0, c0)


@functools.lru_cache(maxsize=None)
def batch_proton(shape):
    """Four studies, float32 [4][R][C][Z], read-only.
    0: a noisy phantom -- a bright elliptical body, two dark lungs whose size changes with the slice,
       Rician background, a few bright vessel pixels in the lungs, a few isolated dark pixels in the body;
    1: a 0 / 1 maze (maze_layout along the longer axis), the corridor closed on odd slices and opened to
       the border by one pixel on even ones; a NaN in the wall between two runs, a -inf in the corridor
       and a +inf in the wall;
    2: all dark under THRESH[2] (uniform noise in [0, 1));
    3: a bright one-pixel frame on the image edge around a dark interior; in one slice two pixels of the
       frame are dark."""
    R, C, Z = shape
    rng = np.random.default_rng(20241101 + R * 1000003 + C * 1009 + Z)
    x = np.zeros((4, R, C, Z), np.float32)
    for z in range(Z):
        f = 0.7 + 0.075 * ((z * 3) % 5)           # 0.7 .. 1.0
        body = _ellipse(R, C, 0.5 * (R - 1), 0.5 * (C - 1), 0.46 * R, 0.46 * C)
        lungs = _ellipse(R, C, 0.5 * (R - 1), 0.30 * (C - 1), 0.30 * R * f, 0.13 * C * f)
        lungs |= _ellipse(R, C, 0.5 * (R - 1) + (z % 2), 0.70 * (C - 1), 0.27 * R * f, 0.13 * C * f)
        lungs &= body
        noise = np.hypot(rng.normal(0, 5, (R, C)), rng.normal(0, 5, (R, C)))
        img = np.where(body & ~lungs, 100 + rng.normal(0, 8, (R, C)), noise)
        inside = np.argwhere(lungs)
        for r, c in inside[rng.choice(len(inside), min(3, len(inside)), replace=False)]:
            img[r, c] = 100.0                                                    # vessels
        flesh = np.argwhere(body & ~lungs)
        for r, c in flesh[rng.choice(len(flesh), min(4, len(flesh)), replace=False)]:
            img[r, c] = 1.0                                                      # specks
        x[0, :, :, z] = img
    L, S = (R, C) if R >= C else (C, R)
    dark, _, wall, corr, _ = maze_layout(L, S)
    for z in range(Z):
        m = (~dark).astype(np.float32)
        if z % 2 == 0:
            m[2, 0] = 0.0                          # the corridor's one opening
        m[wall] = np.nan
        m[corr] = -np.inf
        m[5, S // 2] = np.inf                      # in the wall between the next two runs
        x[1, :, :, z] = m if R >= C else m.T
    x[2] = rng.random((R, C, Z), dtype=np.float32)
    x[3] = rng.random((R, C, Z), dtype=np.float32)
    x[3, 0] = x[3, -1] = 100.0
    x[3, :, 0] = x[3, :, -1] = 100.0
    x[3, 0, 3:5, min(1, Z - 1)] = 0.5
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def batch_stats(shape, n=4):
    """(thresh float32 [n], pmax float32 [n], hist uint32 [n][256]) of batch_proton(shape)[:n]."""
    x = batch_proton(shape)[:n]
    st = [stats(v) for v in x]
    out = (np.array([threshold(v) for v in x], np.float32), np.array([s[0] for s in st], np.float32),
           np.stack([s[1] for s in st]))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def batch_unopened(shape, otsu=False, n=4):
    """The segmentation before the opening, uint8 [n][R][C][Z]: the fill is computed once per shape."""
    x = batch_proton(shape)[:n]
    ts = batch_stats(shape, n)[0] if otsu else THRESH[:n]
    out = batch_segment(x, ts, (0,) * n)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def batch_reference(shape, radii, otsu=False, n=4):
    seg = batch_unopened(shape, otsu, n)
    out = np.stack([M.open_(s, int(k)).astype(np.uint8) if k else s for s, k in zip(seg, radii)])
    out.setflags(write=False)
    return out
