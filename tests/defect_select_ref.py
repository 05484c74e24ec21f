"""Inputs and the CPU reference of the defect-selection tests (test_defect_select_host.py,
test_gpu_defect_select.py): the three thresholdings' raw maps, their medians and borders, the
k-means label map and the cut values, all from oracle.vdp_oracle.  Not a test module."""
import functools

import numpy as np

from oracle import vdp_oracle as O

F32 = np.float32
SOURCES = ("mean", "lb", "kmeans")
SHAPES = [(41, 37, 9), (66, 66, 2), (33, 20, 5), (40, 24, 1), (7, 5, 3)]
VOX = (1.5, 1.5, 10.0)


def field(shape, seed):
    """A smooth noisy field in an elliptic mask: the three thresholdings give three pairwise different
    maps, before and after the median (synth_volume's clean-zero defects give one map for all)."""
    rng = np.random.default_rng(seed)
    f = rng.random(shape)
    for _ in range(3):
        for ax in (0, 1):
            f = (np.roll(f, 1, ax) + f + np.roll(f, -1, ax)) / 3
    f = (f - f.min()) / (f.max() - f.min())
    X = (0.02 + 1.3 * f) * (1 + 0.08 * rng.standard_normal(shape))
    i, j, k = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    R, C, Z = shape
    M = (((i - (R - 1) / 2) / (0.48 * R)) ** 2 + ((j - (C - 1) / 2) / (0.48 * C)) ** 2) <= 1
    return np.abs(X).astype(np.float32), M.astype(np.uint8)


def kmeans_cuts(sig):
    """(cuts 1..3 of kmeans_1d_sorted's final partition, its counts)."""
    counts, _, _ = O.kmeans_1d_sorted(sig)
    return np.cumsum(counts)[:3].astype(np.int64), counts


def labels_by_value(N4, mask, sig, cuts):
    """The value rule: 1 + #{j : cut_j < n and x >= sorted[cut_j]} in the mask, 0 outside."""
    n = sig.shape[0]
    lab = np.ones(N4.shape, np.uint8)
    for c in cuts:
        if c < n:
            lab += N4 >= sig[c]
    return lab * (mask != 0)


def labels_by_index(N4, mask, cuts):
    """The index rule: 1 + the cluster of the voxel's position in the stable-sorted masked list."""
    on = mask != 0
    order = np.argsort(N4[on], kind="stable")
    cl = np.searchsorted(np.asarray(cuts), np.arange(order.size), side="right")
    lab_sorted = np.empty(order.size, np.uint8)
    lab_sorted[order] = 1 + cl
    lab = np.zeros(N4.shape, np.uint8)
    lab[on] = lab_sorted
    return lab


def filtered(raw, medfilt):
    """(defect, border) uint8 of a raw 0/1 map under medfilt 0 / 1 / 2."""
    if medfilt == 0:
        d = raw.astype(np.float64)
    elif medfilt == 1:
        d = O.medfilt3x3_binary(raw)
    else:
        d = O.medfilt3d_binary(raw)
    bo = O.calculate_border3d(d) if medfilt == 2 else O.calculate_border(d)
    return d.astype(np.uint8), (bo == 1).astype(np.uint8)


def reference(N4, mask, thresh=0.6):
    """One study's reference: raw[source] (bool), km (uint8 labels), cuts (float32 [3], +inf where
    the cut is at n), counts (k-means cluster sizes), n_lb12, n_km0."""
    N4 = np.asarray(N4, dtype=F32)
    on = np.asarray(mask) != 0
    zero = np.zeros(N4.shape, bool)
    if not on.any():
        return dict(raw={s: zero for s in SOURCES}, km=np.zeros(N4.shape, np.uint8),
                    cuts=np.full(3, np.inf, F32), counts=np.zeros(4, np.int64), n_lb12=0, n_km0=0)
    sig = np.sort(N4[on], kind="stable")
    m = O.mean_f32(sig)
    raw_mean = ((N4 / m).astype(F32) < F32(thresh)) & on
    p99 = sig[int(len(sig) * .99)]
    lb = O.lb_classes((N4 / p99).astype(F32)) * on
    raw_lb = (lb == 1) | (lb == 2)
    cuts, counts = kmeans_cuts(sig)
    km = labels_by_value(N4, on, sig, cuts)
    low = int(np.flatnonzero(counts > 0)[0])
    raw_km = (km == low + 1) & on
    n = sig.shape[0]
    cutv = np.array([sig[c] if c < n else np.inf for c in cuts], F32)
    return dict(raw={"mean": raw_mean, "lb": raw_lb, "kmeans": raw_km}, km=km, cuts=cutv,
                counts=np.asarray(counts), n_lb12=int(raw_lb.sum()), n_km0=O.kmeans_low_count(counts))


def studies(shape):
    """The batch of a shape: field seeds 1 and 2, an all-zero-mask study, a constant study (every
    masked value 1.0) and a two-valued study (values 1 and 2, mask all ones)."""
    X1, M1 = field(shape, 1)
    X2, M2 = field(shape, 2)
    two = np.where(np.random.default_rng(3).random(shape) < 0.3, 2.0, 1.0).astype(F32)
    hp = np.stack([X1, X2, X1, np.ones(shape, F32), two])
    mk = np.stack([M1, M2, np.zeros(shape, np.uint8), M1, np.ones(shape, np.uint8)])
    return hp, mk


@functools.lru_cache(maxsize=None)
def batch_reference(shape):
    """(hp, mask, [reference(study)]) of studies(shape), computed once and read-only."""
    hp, mk = studies(shape)
    refs = [reference(hp[q], mk[q]) for q in range(hp.shape[0])]
    hp.setflags(write=False)
    mk.setflags(write=False)
    return hp, mk, refs
