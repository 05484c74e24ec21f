"""The numpy reference of the proton resampler (include/vent_hip.h, "the proton resampled from its own
grid"): the tap tables by the formula in float64, three vectorised axis passes with a float32 multiply and
then a float32 add per tap, and a slow per-voxel nested loop for tiny cases; and the seeded phantom the
host and GPU tests share."""
import functools

import numpy as np

TAPS = 8

# the host test's grid of maps
SCALES = (0.25, 0.5, 0.6, 1.0, 1.3, 1.7, 2.0, 3.9, 4.0)


def offsets(n_src):
    """0, fractions of either sign, whole numbers, and one beyond the source."""
    return (0.0, 0.5, -0.4, 2.0, -7.25, float(n_src) + 6.0)


# (source shape, destination shape) -> the maps [(scale, offset) per axis] of studies 0..3
CASES = {
    ((83, 75, 9), (41, 37, 9)): [          # scale near 2 with fractional offsets
        [(2.0, 1.0), (2.0, 1.0), (1.0, 0.0)],
        [(2.0, 0.5), (2.0, 0.5), (1.0, 0.0)],
        [(2.05, 0.3), (1.95, -0.7), (1.0, 0.25)],
        [(1.9, 1.37), (2.1, -1.5), (1.1, -0.4)]],
    ((21, 19, 5), (41, 37, 9)): [          # upsampling on every axis, z included
        [(0.5, 0.0), (0.5, 0.0), (0.5, 0.0)],
        [(0.5, -0.25), (0.5, -0.25), (0.5, -0.25)],
        [(0.45, 0.6), (0.52, -0.3), (0.55, -0.1)],
        [(0.25, 2.0), (0.3, 1.0), (0.4, 0.7)]],
    ((64, 40, 12), (41, 37, 9)): [         # mixed scales; part of the output lies outside the source
        [(1.7, -0.4), (0.6, 0.3), (1.3, 0.2)],
        [(1.7, -7.25), (0.6, -3.0), (1.3, -2.0)],
        [(1.7, 10.0), (0.6, 25.0), (1.3, 4.0)],
        [(4.0, -100.0), (0.6, 0.3), (1.3, 0.2)]],
    ((1, 1, 1), (12, 10, 1)): [
        [(1.0, 0.0), (1.0, 0.0), (1.0, 0.0)],
        [(0.25, -1.0), (0.25, -1.0), (1.0, 0.0)],
        [(4.0, -20.0), (0.5, -2.0), (1.0, 0.3)],
        [(1.0, -5.5), (1.0, -4.5), (1.0, 0.0)]],
    ((256, 256, 24), (128, 128, 24)): [    # the bench shape: studies 0 and 1 only
        [(2.0, 0.5), (2.0, 0.5), (1.0, 0.0)],
        [(2.0, 0.75), (2.0, 0.25), (1.0, 0.0)]],
}


def studies(src_shape):
    return 2 if src_shape == (256, 256, 24) else 4


# ---- the taps of one axis ------------------------------------------------------------------------------
def taps(n_src, n_dst, scale, offset):
    """(first int32 [n_dst], count int32 [n_dst], weight float32 [n_dst][8]) of one axis, every step in
    float64 in the order of the spec."""
    scale, offset = np.float64(scale), np.float64(offset)
    w = max(np.float64(1.0), scale)
    first, count = np.zeros(n_dst, np.int32), np.zeros(n_dst, np.int32)
    weight = np.zeros((n_dst, TAPS), np.float32)
    for i in range(n_dst):
        u = scale * np.float64(i) + offset
        js, ts = [], []
        for j in range(int(np.floor(u - w)) - 2, int(np.ceil(u + w)) + 3):
            t = np.float64(1.0) - np.abs(np.float64(j) - u) / w
            if t > 0:
                js.append(j)
                ts.append(t)
        assert len(js) <= TAPS and js == list(range(js[0], js[0] + len(js)))
        W = np.float64(0.0)
        for t in ts:
            W = W + t
        k = 0
        for j, t in zip(js, ts):
            if 0 <= j < n_src:
                if k == 0:
                    first[i] = j
                weight[i, k] = np.float32(t / W)
                k += 1
        count[i] = k
    return first, count, weight


def tables(src_shape, dst_shape, m):
    """The three tables of one study's map [3][2]."""
    return [taps(src_shape[a], dst_shape[a], m[a][0], m[a][1]) for a in range(3)]


# ---- the value, three vectorised passes ---------------------------------------------------------------
def _axis_pass(x, table, axis):
    """out[.., i, ..] = the sum over the taps of i, ascending, of weight * x[.., first + k, ..]: a float32
    multiply, then a float32 add, starting from +0.0f."""
    first, count, weight = table
    x = np.moveaxis(np.asarray(x, np.float32), axis, -1)
    acc = np.zeros(x.shape[:-1] + (len(first),), np.float32)
    n = x.shape[-1]
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(int(count.max()) if len(count) else 0):
            on = k < count
            term = (weight[:, k] * x[..., np.clip(first + k, 0, n - 1)]).astype(np.float32)
            acc = np.where(on, (acc + term).astype(np.float32), acc)
    return np.moveaxis(acc, -1, axis)


def resample(src, dst_shape, m):
    """One study, float32 [Rs][Cs][Zs] -> float32 dst_shape, with the map m [3][2]: the z-pass, the
    c-pass, the r-pass (the nested sum of the spec is exactly separable)."""
    tr, tc, tz = tables(np.shape(src), dst_shape, m)
    return _axis_pass(_axis_pass(_axis_pass(src, tz, 2), tc, 1), tr, 0)


def resample_nested(src, dst_shape, m):
    """The same a voxel at a time, exactly as the spec writes it (tiny cases only)."""
    src = np.asarray(src, np.float32)
    (fr, kr, wr), (fc, kc, wc), (fz, kz, wz) = tables(src.shape, dst_shape, m)
    out = np.zeros(dst_shape, np.float32)
    zero = np.float32(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(dst_shape[0]):
            for c in range(dst_shape[1]):
                for z in range(dst_shape[2]):
                    ar = zero
                    for a in range(kr[r]):
                        ac = zero
                        for b in range(kc[c]):
                            az = zero
                            for d in range(kz[z]):
                                az = np.float32(az + np.float32(wz[z, d] * src[fr[r] + a, fc[c] + b, fz[z] + d]))
                            ac = np.float32(ac + np.float32(wc[c, b] * az))
                        ar = np.float32(ar + np.float32(wr[r, a] * ac))
                    out[r, c, z] = ar
    return out


# ---- the phantom ---------------------------------------------------------------------------------------
def study(shape, seed):
    """A proton float32 of ``shape``: a bright smooth body, two dark lungs that vary with the slice, a
    gradient along the rows, Rician-like noise."""
    rng = np.random.default_rng(seed)
    R, C, Z = shape
    r, c, z = np.meshgrid(np.arange(R), np.arange(C), np.arange(Z), indexing="ij")
    u, w = (r - (R - 1) / 2) / max(R, 2), (c - (C - 1) / 2) / max(C, 2)
    t = (z - (Z - 1) / 2) / max(Z, 2)
    grow = 1.0 - 1.6 * t * t + 0.3 * t
    soft = lambda d: 1.0 / (1.0 + np.exp(np.clip((d - 1.0) * 12.0, -60, 60)))   # noqa: E731  1 inside, 0 outside
    body = soft((u / 0.38) ** 2 + (w / 0.34) ** 2)
    lungs = np.maximum(soft((u / (0.24 * grow)) ** 2 + ((w + 0.16) / (0.10 * grow)) ** 2),
                       soft(((u - 0.03) / (0.21 * grow)) ** 2 + ((w - 0.17) / (0.11 * grow)) ** 2))
    signal = body * (100.0 + 30.0 * (u + 0.5)) * (1.0 - 0.88 * lungs)
    img = np.sqrt((signal + rng.normal(0, 4.0, shape)) ** 2 + rng.normal(0, 4.0, shape) ** 2)
    return img.astype(np.float32)


def default_maps(src_shape, dst_shape, n):
    """Centre on centre at the ratio of the shapes (clipped to the limits), each study a little off."""
    out = []
    for q in range(n):
        m = []
        for a in range(3):
            s = min(4.0, max(0.25, src_shape[a] / dst_shape[a]))
            m.append((s, (src_shape[a] - 1) / 2 - s * (dst_shape[a] - 1) / 2 + 0.3 * q * (1 - a)))
        out.append(m)
    return out


@functools.lru_cache(maxsize=None)
def batch(src_shape, dst_shape):
    """(source float32 [n][Rs][Cs][Zs], maps float64 [n][3][2]), read-only: n = studies(src_shape)
    studies with the maps of CASES (default_maps for a pair of shapes it does not list)."""
    n = studies(src_shape)
    maps = CASES.get((src_shape, dst_shape)) or default_maps(src_shape, dst_shape, n)
    S = np.stack([study(src_shape, 100 * q + sum(src_shape)) for q in range(n)])
    M = np.asarray(maps[:n], np.float64)
    S.setflags(write=False)
    M.setflags(write=False)
    return S, M


def reference_of(S, maps, dst_shape):
    return np.stack([resample(s, dst_shape, m) for s, m in zip(S, maps)])


@functools.lru_cache(maxsize=None)
def reference(src_shape, dst_shape):
    """float32 [n][R][C][Z] of batch(src_shape, dst_shape), read-only."""
    S, M = batch(src_shape, dst_shape)
    out = reference_of(S, M, dst_shape)
    out.setflags(write=False)
    return out
