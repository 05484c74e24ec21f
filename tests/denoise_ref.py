"""Inputs and the numpy reference of the denoise tests (test_denoise_host.py, test_gpu_denoise.py):
the in-plane non-local-means filter and the noise estimate exactly as include/vent_hip.h specifies
them, vectorised over shifted windows of the edge-padded volume, float32 throughout, the loops in the
stated order.  numpy rounds every elementwise float32 operation on its own (no fused multiply-add),
which is the arithmetic the kernel is held to.  Not a test module."""
import functools

import numpy as np

from oracle import vdp_oracle as O

F32 = np.float32
SHAPES = [(5, 7, 3), (41, 37, 9), (64, 64, 24), (130, 19, 2)]   # slice < halo; odd tile remainders;
                                                                # whole tiles; tall and thin
PARAMS = ((3, 1), (1, 0), (5, 2))                               # (search, patch)
SIGMAS = (F32(9.5), F32(23.25), F32(4.125))                     # one per study of a batch
STRENGTH = 2.0
VOX = (1.5, 1.5, 10.0)


def constants(sigma, strength, patch):
    """(inv_h2, bias) of one study: in double from the float32 sigma and strength, rounded to float32
    once.  inv_h2 = 1 / (2 n (k sigma)^2) with n = (2 patch + 1)^2; bias = 2 sigma^2."""
    s, k = np.float64(F32(sigma)), np.float64(F32(strength))
    n = np.float64((2 * int(patch) + 1) ** 2)
    ks = k * s
    with np.errstate(divide="ignore", over="ignore"):
        return F32(np.float64(1.0) / (2.0 * n * (ks * ks))), F32(2.0 * (s * s))


def denoise(x, sigma, strength=STRENGTH, search=3, patch=1, rician=False):
    """The filter on one study x float32 [R][C][Z]; returns float32 [R][C][Z]."""
    x = np.asarray(x)
    assert x.dtype == F32 and x.ndim == 3
    S, P = int(search), int(patch)
    R, C, _ = x.shape
    H = S + P
    inv_h2, bias = constants(sigma, strength, P)
    xp = np.pad(x, ((H, H), (H, H), (0, 0)), mode="edge")

    def win(dr, dc):   # X(r + dr, c + dc) for every voxel
        return xp[H + dr:H + dr + R, H + dc:H + dc + C]

    num = np.zeros(x.shape, F32)
    den = np.zeros(x.shape, F32)
    one = F32(1)
    with np.errstate(all="ignore"):
        for dr in range(-S, S + 1):
            for dc in range(-S, S + 1):
                d2 = np.zeros(x.shape, F32)
                for ur in range(-P, P + 1):
                    for uc in range(-P, P + 1):
                        t = win(ur, uc) - win(dr + ur, dc + uc)
                        d2 = d2 + t * t
                u = d2 * inv_h2
                v = one - u
                w = np.where(u < one, v * v, F32(0))
                y = win(dr, dc)
                if rician:
                    y = y * y
                num = num + w * y
                den = den + w
        out = num / den
        if rician:
            v = out - bias
            out = np.where(v > 0, np.sqrt(v), F32(0))
    assert out.dtype == F32
    return out


def sigma_of(noise):
    """float32(sqrt(S2 / (2 N))) over the given background values (sums in double); NaN for none."""
    v = np.asarray(noise, dtype=np.float64).ravel()
    if v.size == 0:
        return F32(np.nan)
    return F32(np.sqrt(np.sum(v * v) / (2.0 * v.size)))


def noise_sigma(hp, mask):
    """The estimate over exactly calculate_SNR's noise voxels (oracle.vdp_oracle.noise_mask); NaN
    where the reference would raise (no masked column > 0) or the noise region is empty."""
    mask = np.asarray(mask)
    cols = (mask != 0).sum(axis=(0, 2)) > 0
    if not cols[1:].any():
        return F32(np.nan)
    return sigma_of(np.asarray(hp, dtype=F32)[O.noise_mask((mask != 0).astype(np.float64))])


def field(shape, seed):
    """Seeded positive floats with structure (a smooth ramp, blocks, noise) so that the weights take
    values across (0, 1] and exact zeros; float32 [R][C][Z]."""
    R, C, Z = shape
    rng = np.random.default_rng(seed)
    i, j, k = np.meshgrid(np.arange(R), np.arange(C), np.arange(Z), indexing="ij")
    x = 60.0 + 40.0 * np.sin(i / 5.0 + seed) * np.cos(j / 7.0) + 25.0 * ((i // 6 + j // 5 + k) % 3)
    x = x + rng.rayleigh(10.0 + 5.0 * seed, shape)
    return np.abs(x).astype(F32) + F32(0.5)


def ellipse(shape, frac):
    """uint8 0/1: the in-plane ellipse of semi-axes frac * (R, C) about the centre, on every slice."""
    R, C, Z = shape
    i, j, _ = np.meshgrid(np.arange(R), np.arange(C), np.arange(Z), indexing="ij")
    return ((((i - (R - 1) / 2) / (frac * R)) ** 2 + ((j - (C - 1) / 2) / (frac * C)) ** 2) <= 1).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def batch_inputs(shape):
    """hp float32 [3][R][C][Z]: two seeded fields and an all-zero study; read-only."""
    hp = np.stack([field(shape, 1), field(shape, 2), np.zeros(shape, F32)])
    hp.setflags(write=False)
    return hp


@functools.lru_cache(maxsize=None)
def batch_masks(shape):
    """uint8 [3][R][C][Z]: a wide ellipse, a narrow one, an empty mask (its noise estimate is NaN);
    read-only."""
    mk = np.stack([ellipse(shape, 0.45), ellipse(shape, 0.3), np.zeros(shape, np.uint8)])
    mk.setflags(write=False)
    return mk


@functools.lru_cache(maxsize=None)
def batch_reference(shape, search, patch, rician):
    """denoise() of every study of batch_inputs(shape) with SIGMAS, computed once; read-only."""
    hp = batch_inputs(shape)
    out = np.stack([denoise(hp[q], SIGMAS[q], STRENGTH, search, patch, rician) for q in range(hp.shape[0])])
    out.setflags(write=False)
    return out


# ---- the phantom of the recovery test -------------------------------------------------------------
def phantom(shape=(64, 64, 6)):
    """(clean float32, mask bool): the two-ellipsoid mask of the synthetic generator,
    exp(0.4 (i - R/2) / R) * 200 inside it, 0 outside, and one in-plane disc defect of radius 4
    (every slice) at 0.2 of the signal."""
    R, C, Z = shape
    i, j, k = np.meshgrid(np.arange(R, dtype=np.float64), np.arange(C, dtype=np.float64),
                          np.arange(Z, dtype=np.float64), indexing="ij")
    m = np.zeros(shape, bool)
    for cc in (0.32, 0.68):
        m |= (((i - 0.5 * R) / (0.35 * R)) ** 2 + ((j - cc * C) / (0.17 * C)) ** 2
              + ((k - 0.5 * Z) / (0.42 * Z)) ** 2) <= 1
    x = np.exp(0.4 * (i - R / 2) / R) * 200 * m
    disc = ((i - 0.45 * R) ** 2 + (j - 0.32 * C) ** 2 <= 16) & m
    x[disc] *= 0.2
    return x.astype(F32), m


def noisy(clean, sigma, seed=0):
    """|clean + complex Gaussian noise of standard deviation sigma per channel|, float32."""
    rng = np.random.default_rng(seed)
    re = clean + rng.normal(0.0, sigma, clean.shape)
    im = rng.normal(0.0, sigma, clean.shape)
    return np.hypot(re, im).astype(F32)
