"""Inputs and the numpy reference of the heterogeneity tests (test_heterogeneity_host.py,
test_gpu_heterogeneity.py): the local coefficient of variation and its summary exactly as
include/vent_hip.h specifies them, vectorised over shifted windows of the zero-padded volume and mask,
float32 throughout, the loops in the stated order, the conditional adds as np.where(w, s + x, s).  numpy
rounds every elementwise float32 operation on its own (no fused multiply-add), which is the arithmetic
the kernel is held to.  Not a test module."""
import functools

import numpy as np

import denoise_ref as D

F32 = np.float32
SHAPES = D.SHAPES                        # slice < halo; odd tile remainders; whole tiles; tall and thin
PARAMS = ((1, 2), (2, 13), (5, 2))       # (radius, min_count)
BINS, HI = 64, 0.5
FX = F32(16777216.0)                     # 2^24: the fixed-point scale of the sum


def cov_map(x, M, radius, min_count):
    """The map of one study: x float32 [R][C][Z], M bool [R][C][Z] the effective mask; float32
    [R][C][Z]: +0 where M is clear, -1 where it is set but there is no value, else cv."""
    x = np.asarray(x)
    M = np.asarray(M)
    assert x.dtype == F32 and x.ndim == 3 and M.dtype == np.bool_ and M.shape == x.shape
    k = int(radius)
    R, C, _ = x.shape
    xp = np.pad(x, ((k, k), (k, k), (0, 0)))          # (the padding is never counted: its mask is clear)
    mp = np.pad(M, ((k, k), (k, k), (0, 0)))
    offs = [(dr, dc) for dr in range(-k, k + 1) for dc in range(-k, k + 1)]

    def win(a, dr, dc):   # a(r + dr, c + dc) for every voxel
        return a[k + dr:k + dr + R, k + dc:k + dc + C]

    n = np.zeros(x.shape, np.int32)
    s = np.zeros(x.shape, F32)
    with np.errstate(all="ignore"):
        for dr, dc in offs:
            w = win(mp, dr, dc)
            n = n + w
            s = np.where(w, s + win(xp, dr, dc), s)
        m = s / n.astype(F32)
        q = np.zeros(x.shape, F32)
        for dr, dc in offs:
            t = win(xp, dr, dc) - m
            q = np.where(win(mp, dr, dc), q + t * t, q)
        has = (n >= int(min_count)) & (m > 0)
        cv = np.sqrt(q / (n - 1).astype(F32)) / m
    out = np.where(M, np.where(has, cv, F32(-1)), F32(0))
    assert out.dtype == F32
    return out


def summary(out, M, bins=BINS, hi=HI):
    """(hist uint32 [bins], stats int64 [4] = n_in, n_over, n_none, sum_fx) of one study's map."""
    hi = F32(hi)
    scale = F32(bins) / hi
    assert scale.dtype == F32
    M = np.asarray(M)
    v = out[M]
    none = v == F32(-1)          # (a cv is never negative: a root over a positive mean)
    cv = v[~none]
    with np.errstate(invalid="ignore"):
        inside = cv < hi         # (NaN: outside)
    ci = cv[inside]
    prod = ci * scale
    fx = ci * FX
    assert prod.dtype == F32 and fx.dtype == F32
    b = np.minimum(bins - 1, prod.astype(np.int64))
    hist = np.bincount(b, minlength=bins).astype(np.uint32)
    stats = np.array([ci.size, cv.size - ci.size, int(none.sum()), int(fx.astype(np.int64).sum())], np.int64)
    return hist, stats


def index(stats):
    """sum_fx / 2^24 / n_in in double; NaN for n_in == 0."""
    return float(stats[3]) / 16777216.0 / float(stats[0]) if stats[0] else float("nan")


def holes(shape, seed, frac=0.15):
    """bool [R][C][Z]: True where a seeded draw leaves the mask standing (about 1 - frac of the voxels)."""
    return np.random.default_rng(seed).random(shape) >= frac


@functools.lru_cache(maxsize=None)
def batch_inputs(shape):
    """x float32 [3][R][C][Z]: a structured positive field; the same kind of field set to exactly 0
    inside a small central ellipse (the mean is 0 deep inside it: no value; tiny at its rim: a huge
    cv); another field, under the empty mask.  Read-only."""
    x1 = D.field(shape, 2).copy()
    x1[D.ellipse(shape, 0.2) != 0] = F32(0)
    x = np.stack([D.field(shape, 1), x1, D.field(shape, 3)])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def batch_masks(shape):
    """uint8 [3][R][C][Z]: a wide ellipse and a narrow one, each with about 15 % seeded holes, and an
    empty mask.  Read-only."""
    mk = np.stack([D.ellipse(shape, 0.45) * holes(shape, 11), D.ellipse(shape, 0.3) * holes(shape, 12),
                   np.zeros(shape, np.uint8)]).astype(np.uint8)
    mk.setflags(write=False)
    return mk


def reference(x, M, radius, min_count, bins=BINS, hi=HI):
    """(map [B][R][C][Z], hist [B][bins], stats [B][4]) of a batch x with effective masks M (bool)."""
    maps = np.stack([cov_map(x[q], M[q], radius, min_count) for q in range(x.shape[0])])
    sm = [summary(maps[q], M[q], bins, hi) for q in range(x.shape[0])]
    return maps, np.stack([h for h, _ in sm]), np.stack([s for _, s in sm])


@functools.lru_cache(maxsize=None)
def batch_reference(shape, radius, min_count):
    """reference() of batch_inputs(shape) under batch_masks(shape), computed once; read-only."""
    out = reference(batch_inputs(shape), batch_masks(shape) != 0, radius, min_count)
    for a in out:
        a.setflags(write=False)
    return out
