"""The numpy reference of the mask edits (include/vent_hip.h, "editing the masks of a device-resident
batch"): per-slice disc erosion, dilation, opening and closing by direct shifts over a padded array,
and the paint strokes; and the seeded inputs the host and GPU tests share.  No scipy here: the host
test compares this file against scipy.ndimage."""
import functools

import numpy as np

OPS = ("erode", "dilate", "open", "close")
HOWS = ("or", "andnot", "and", "xor")
SHAPES = [(5, 7, 3), (12, 9, 1), (41, 37, 9), (64, 64, 24), (130, 19, 2), (33, 40, 33)]
RADII = [(1, 2, 5, 3), (5, 1, 4, 2), (3, 0, 3, 0)]   # one radius per study of batch_masks


def disc(k):
    """The offsets (dr, dc) of D_k = {dr^2 + dc^2 <= k^2}: 5, 13, 29, 49, 81 of them for k = 1..5."""
    return [(dr, dc) for dr in range(-k, k + 1) for dc in range(-k, k + 1) if dr * dr + dc * dc <= k * k]


def _sweep(s, k, pad):
    """OR (pad 0) or AND (pad 1) over D_k of the bool volume s [R][C][Z], every slice on its own; a
    position outside the slice counts as ``pad``."""
    R, C, _ = s.shape
    p = np.pad(s, ((k, k), (k, k), (0, 0)), constant_values=bool(pad))
    out = np.full(s.shape, bool(pad))
    for dr, dc in disc(k):
        v = p[k + dr:k + dr + R, k + dc:k + dc + C]
        out = (out & v) if pad else (out | v)
    return out


def dilate(s, k):
    return _sweep(np.asarray(s) != 0, k, 0)


def erode(s, k):
    return _sweep(np.asarray(s) != 0, k, 1)


def open_(s, k):
    return dilate(erode(s, k), k)      # the intermediate lives on the slice: dilate pads it with 0


def close(s, k):
    return erode(dilate(s, k), k)      # ... and erode pads it with 1


_FN = dict(erode=erode, dilate=dilate, open=open_, close=close)


def edit(mask, op, radius):
    """One study, uint8 [R][C][Z] -> uint8: 0 / 1 bytes, or the mask as it is for radius 0."""
    mask = np.asarray(mask)
    if radius == 0:
        return mask.astype(np.uint8)
    return _FN[op](mask, int(radius)).astype(np.uint8)


def batch_edit(masks, op, radii):
    return np.stack([edit(m, op, r) for m, r in zip(masks, radii)])


def paint(mask, strokes, how):
    s, p = np.asarray(mask) != 0, np.asarray(strokes) != 0
    out = {"or": s | p, "andnot": s & ~p, "and": s & p, "xor": s ^ p}[how]
    return out.astype(np.uint8)


def _ellipse(R, C, r0, c0, a, b):
    rr, cc = np.mgrid[0:R, 0:C]
    return ((rr - r0) / max(a, 0.5)) ** 2 + ((cc - c0) / max(b, 0.5)) ** 2 <= 1.0


@functools.lru_cache(maxsize=None)
def batch_masks(shape):
    """Four studies, uint8 [4][R][C][Z], read-only.  Every shape changes from slice to slice (scaled
    and shifted with z), so a slice mix-up in the packing shows.
    0: values 0/1 -- two in-plane ellipses joined by a 2-pixel bridge, with one-voxel holes, a
       one-pixel-wide slit and isolated one- and two-voxel specks outside;
    1: values 0/2/255 -- a blob clipped by row 0 and one clipped by the last column, with holes;
    2: empty;   3: all ones."""
    R, C, Z = shape
    rng = np.random.default_rng(20241023 + R * 1000003 + C * 1009 + Z)
    m = np.zeros((4, R, C, Z), np.uint8)
    for z in range(Z):
        f = 0.8 + 0.05 * ((z * 3) % 5)          # 0.8 .. 1.0
        dr = (z % 3) - 1                          # the rows shift by -1, 0, 1
        rc = 0.5 * (R - 1) + dr
        a = _ellipse(R, C, rc, 0.27 * (C - 1), 0.40 * R * f, 0.19 * C * f)
        a |= _ellipse(R, C, rc, 0.73 * (C - 1), 0.36 * R * f, 0.19 * C * f)
        ri = int(round(rc))
        if 0 <= ri and ri + 2 <= R:
            a[ri:ri + 2, int(0.27 * (C - 1)):int(0.73 * (C - 1)) + 1] = True      # the bridge
        inside = np.argwhere(a)
        if len(inside) > 8:
            for r, c in inside[rng.choice(len(inside), 4, replace=False)]:
                a[r, c] = False                                                   # one-voxel holes
        cs = int(0.27 * (C - 1)) + (z % 2)
        a[max(ri - R // 5, 0):ri - 1, cs] = False                                 # the slit
        a[0, 0] = True                                                            # specks
        a[R - 1, C - 2:C] = True
        if R > 8 and C > 8:
            a[1 + z % 2, C // 2] = True
        m[0, :, :, z] = a
        b = _ellipse(R, C, 0, 0.3 * (C - 1) + dr, 0.45 * R * f, 0.24 * C * f)
        d = _ellipse(R, C, 0.62 * (R - 1), C - 1, 0.30 * R * f, 0.42 * C * f)
        v = np.where(d, 255, np.where(b, 2, 0)).astype(np.uint8)
        inside = np.argwhere(v)
        if len(inside) > 8:
            for r, c in inside[rng.choice(len(inside), 4, replace=False)]:
                v[r, c] = 0
        m[1, :, :, z] = v
    m[3] = 1
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def batch_reference(shape, op, radii):
    out = batch_edit(batch_masks(shape), op, radii)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def batch_strokes(shape):
    """Strokes in {0, 7, 255}, uint8 [4][R][C][Z]: scattered voxels, and one run of the flat buffer
    that crosses the boundary between studies 0 and 1 (and the one between 2 and 3)."""
    rng = np.random.default_rng(7 + int(np.prod(shape)))
    s = rng.choice(np.array([0, 0, 0, 7, 255], np.uint8), size=(4,) + tuple(shape))
    V = int(np.prod(shape))
    flat = s.reshape(-1)
    for q in (1, 3):
        flat[q * V - 9:q * V + 11] = 255
    s.setflags(write=False)
    return s
