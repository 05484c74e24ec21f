"""Inputs and the numpy reference of the distribution tests (test_distribution_host.py,
test_gpu_distribution.py): per study the histogram of the normalised masked signal and the slice
counts of mask, defect and linear-binning class voxels, with the mean anchor, the 99th percentile and
the classes of oracle.vdp_oracle.  Every value is an integer.  Not a test module."""
import functools

import numpy as np

from oracle import vdp_oracle as O

import defect_select_ref as D

F32 = np.float32
COLS = 8
SHAPES = D.SHAPES
TALL = (12, 10, 300)          # more slices than a workgroup has threads: the LDS slice counters
PARAMS = ((1024, 1.5), (100, 1.5), (1, 0.5), (7, 2.0))
NORMS = ("mean", "p99")
VOX = D.VOX


def studies(shape):
    """defect_select_ref.studies(shape) -- two fields, an empty mask, a constant study, a two-valued
    study -- plus the seed-2 field with a few masked values negated (they land in outside[0]) and the
    seed-1 field with every masked value 0 (d = 0: NaN fills outside[1])."""
    hp, mk = D.studies(shape)
    neg = hp[1].copy()
    idx = np.flatnonzero(mk[1])
    pick = idx[np.random.default_rng(5).choice(idx.size, size=min(7, idx.size), replace=False)]
    neg.reshape(-1)[pick] *= F32(-0.5)
    zero = np.where(mk[0] != 0, F32(0), hp[0]).astype(F32)
    return (np.concatenate([hp, neg[None], zero[None]]),
            np.concatenate([mk, mk[1][None], mk[0][None]]))


def anchors(N4, mask):
    """(mean_anchor, p99) of a study as calculate_VDP forms them; (None, None) for an empty mask."""
    on = np.asarray(mask) != 0
    if not on.any():
        return None, None
    sig = np.sort(np.asarray(N4, dtype=F32)[on], kind="stable")
    return O.mean_f32(sig), sig[int(len(sig) * .99)]


def lb_volume(N4, mask):
    """The run's LB class volume: uint8 0 off-mask (and for NaN), else the class 1..6."""
    on = np.asarray(mask) != 0
    _, p99 = anchors(N4, mask)
    if p99 is None:
        return np.zeros(np.shape(N4), np.uint8)
    with np.errstate(divide="ignore", invalid="ignore"):
        return O.lb_classes((np.asarray(N4, dtype=F32) / p99).astype(F32)) * on


def run_defect(N4, mask, thresh=0.6):
    """The plain run's defect map: float32(N4 / mean) < thresh in the mask, per-slice 3x3 median."""
    on = np.asarray(mask) != 0
    m, _ = anchors(N4, mask)
    if m is None:
        return np.zeros(np.shape(N4), np.uint8)
    with np.errstate(divide="ignore", invalid="ignore"):
        raw = ((np.asarray(N4, dtype=F32) / m).astype(F32) < F32(thresh)) & on
    return D.filtered(raw, 1)[0]


def histogram(N4, mask, norm, bins, hi):
    """(hist uint32 [bins], outside int64 [2]) of one study: nv = float32(x / d) over mask != 0; the
    bin is min(bins - 1, int(float32(nv * scale))) for 0 <= nv < hi with scale = float32(bins) /
    float32(hi); nv < 0 counts in outside[0], everything else (nv >= hi, NaN) in outside[1]."""
    on = np.asarray(mask) != 0
    m, p99 = anchors(N4, mask)
    if m is None:
        return np.zeros(bins, np.uint32), np.zeros(2, np.int64)
    d = F32(m if norm in ("mean", 0) else p99)
    with np.errstate(divide="ignore", invalid="ignore"):
        nv = (np.asarray(N4, dtype=F32)[on] / d).astype(F32)
    inside = (nv >= 0) & (nv < F32(hi))
    scale = F32(F32(bins) / F32(hi))
    bi = np.minimum(bins - 1, (nv[inside] * scale).astype(F32).astype(np.int64))
    hist = np.bincount(bi, minlength=bins).astype(np.uint32)
    below = int((nv < 0).sum())
    return hist, np.array([below, nv.size - int(inside.sum()) - below], np.int64)


def slice_counts(mask, defect, lb):
    """int64 [Z][8] over all voxels of each slice: mask != 0, defect != 0 (not ANDed with the mask),
    lb == 1 .. 6."""
    cols = [np.asarray(mask) != 0, np.asarray(defect) != 0] + [np.asarray(lb) == c for c in range(1, 7)]
    return np.stack([c.sum(axis=(0, 1)) for c in cols], axis=1).astype(np.int64)


def reference(N4, mask, defect, lb, norm, bins, hi):
    hist, outside = histogram(N4, mask, norm, bins, hi)
    return dict(hist=hist, outside=outside, slice_counts=slice_counts(mask, defect, lb))


@functools.lru_cache(maxsize=None)
def batch_inputs(shape):
    """(hp, mask, defect, lb) of studies(shape) after a plain run with N4 = identity, computed once
    and read-only."""
    hp, mk = studies(shape)
    defect = np.stack([run_defect(x, m) for x, m in zip(hp, mk)]).astype(np.uint8)
    lb = np.stack([lb_volume(x, m) for x, m in zip(hp, mk)]).astype(np.uint8)
    for a in (hp, mk, defect, lb):
        a.setflags(write=False)
    return hp, mk, defect, lb


@functools.lru_cache(maxsize=None)
def batch_reference(shape, norm, bins, hi):
    """[reference(study)] of batch_inputs(shape), computed once."""
    hp, mk, defect, lb = batch_inputs(shape)
    return [reference(hp[q], mk[q], defect[q], lb[q], norm, bins, hi) for q in range(hp.shape[0])]


def assert_equal(got, refs, studies_=None):
    """Batch.download_distribution's dict against the per-study references, exactly."""
    for q, r in enumerate(refs):
        if studies_ is not None and q not in studies_:
            continue
        for k in ("hist", "outside", "slice_counts"):
            assert got[k][q].dtype == r[k].dtype, (k, got[k].dtype)
            assert np.array_equal(got[k][q], r[k]), (q, k, got[k][q], r[k])
