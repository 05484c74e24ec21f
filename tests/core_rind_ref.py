"""The numpy reference of the core-rind analysis (include/vent_hip.h, "the core-rind analysis of a
device-resident batch"): the exact squared in-plane distance of every mask voxel to the nearest clear
pixel of its slice (the one-pixel ring outside the slice is clear), the depth bands and their counts;
and the seeded inputs the host and GPU tests share.  Integers throughout.  No scipy here: the host test
compares this file against scipy.ndimage."""
import functools

import numpy as np

import mask_edit_ref as ME

SHAPES = [(5, 7, 3), (12, 9, 1), (41, 37, 9), (64, 64, 24), (130, 19, 2), (33, 40, 33), (300, 280, 2)]
# no band edge; the one-pixel rind (D2 = 1); depth_thresholds((1.5, 3.5, 8)); 1..31, whose t[0] = 1
# leaves band 0 always empty
THRESHOLDS = [(), (2,), (3, 13, 64), tuple(range(1, 32))]
N_STUDIES = 5
LONG_ROW = (4, 62, 1000)   # a row of 62 000 column distances: past what the search stages in LDS


def d2_slice(M, edge_only=True, chunk=1 << 22):
    """int64 [R][C]: for every set pixel of the bool slice M the minimum over the clear pixels, ring
    included, of the squared offset; 0 where M is clear.  A direct minimum, chunked over the set pixels
    so the table of offsets stays below ``chunk`` entries.

    ``edge_only`` keeps of the clear pixels only those with a set 4-neighbour.  The minimum is the same:
    let q be a nearest clear pixel of the set pixel p, and step from q one pixel towards p along the
    axis on which they differ most.  The step lands strictly nearer to p, so it is not clear: it is a
    set pixel (p itself at the last), and q is its 4-neighbour.  test_core_rind_host checks the two
    against each other."""
    R, C = M.shape
    P = np.zeros((R + 2, C + 2), bool)
    P[1:-1, 1:-1] = M
    clear = ~P
    if edge_only:
        near = np.zeros_like(P)
        near[1:] |= P[:-1]
        near[:-1] |= P[1:]
        near[:, 1:] |= P[:, :-1]
        near[:, :-1] |= P[:, 1:]
        clear &= near
    q = np.argwhere(clear).astype(np.int64) - 1      # slice coordinates; the ring is at -1, R and C
    p = np.argwhere(M).astype(np.int64)
    out = np.zeros((R, C), np.int64)
    if len(p) == 0:
        return out
    step = max(1, chunk // max(len(q), 1))
    for i in range(0, len(p), step):
        s = p[i:i + step]
        d = (s[:, None, 0] - q[None, :, 0]) ** 2 + (s[:, None, 1] - q[None, :, 1]) ** 2
        out[s[:, 0], s[:, 1]] = d.min(axis=1)
    return out


def d2_volume(mask, edge_only=True):
    """int64 [R][C][Z], every slice on its own; ``mask`` of any dtype, nonzero set."""
    M = np.asarray(mask) != 0
    return np.stack([d2_slice(M[:, :, z], edge_only) for z in range(M.shape[2])], axis=2)


def summary(d2, M, D, thr):
    """(counts int64 [len(thr) + 1][2], stats int64 [2]) of one study: d2 int64, M and D bool."""
    thr = np.asarray(thr, dtype=np.int64)
    band = np.searchsorted(thr, np.minimum(d2, 65535)[M], side='right')
    nb = len(thr) + 1
    counts = np.zeros((nb, 2), np.int64)
    counts[:, 0] = np.bincount(band, minlength=nb)
    counts[:, 1] = np.bincount(band[D[M]], minlength=nb)
    stats = np.array([M.sum(), d2.max() if M.any() else 0], np.int64)
    return counts, stats


def reference(masks, defects, thr, d2=None):
    """(map uint16 [B][R][C][Z], counts int64 [B][bands][2], stats int64 [B][2]); ``defects`` None: the
    defect column is 0; ``d2`` the studies' d2_volume when the caller has them already."""
    masks = np.asarray(masks)
    if d2 is None:
        d2 = np.stack([d2_volume(m) for m in masks])
    M = masks != 0
    D = np.zeros_like(M) if defects is None else np.asarray(defects) != 0
    cs = [summary(d2[q], M[q], D[q], thr) for q in range(len(masks))]
    return (np.minimum(d2, 65535).astype(np.uint16), np.stack([c[0] for c in cs]), np.stack([c[1] for c in cs]))


@functools.lru_cache(maxsize=None)
def batch_masks(shape):
    """Five studies, uint8 [5][R][C][Z], read-only: the four of mask_edit_ref.batch_masks (ellipses with
    holes, slits and specks; blobs cut by the slice border in values 0/2/255; empty; all ones), and 4:
    all ones but for one clear pixel in a corner of one slice."""
    R, C, Z = shape
    m = np.empty((N_STUDIES,) + tuple(shape), np.uint8)
    m[:4] = ME.batch_masks(shape)
    m[4] = 1
    m[4, R - 1, 0, Z // 2] = 0
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def batch_defects(shape):
    """uint8 [5][R][C][Z] in {0, 1, 255}, read-only: a seeded 15 % of every mask, and up to eight
    defect voxels off every mask, which no band counts (study 4: its one clear pixel; the full study 3
    has none)."""
    mk = batch_masks(shape) != 0
    rng = np.random.default_rng(977 + int(np.prod(shape)))
    d = ((rng.random(mk.shape) < 0.15) & mk).astype(np.uint8)
    d[rng.random(mk.shape) < 0.05] *= 255
    for q in range(N_STUDIES):
        off = np.argwhere(~mk[q])
        pick = off[rng.choice(len(off), min(len(off), 8), replace=False)]
        d[q][tuple(pick.T)] = 255 if q == 4 else 1
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def batch_d2(shape):
    d2 = np.stack([d2_volume(m) for m in batch_masks(shape)])
    d2.setflags(write=False)
    return d2


@functools.lru_cache(maxsize=None)
def batch_reference(shape, thr, with_defect=True):
    out = reference(batch_masks(shape), batch_defects(shape) if with_defect else None, thr, batch_d2(shape))
    for a in out:
        a.setflags(write=False)
    return out


def border_free(masks, k):
    """The masks with everything within k + 1 pixels of the slice border cleared (0 / 1 bytes): on these
    {D2 > k^2} = erode(mask, k), whatever the padding."""
    m = (np.asarray(masks) != 0).astype(np.uint8)
    e = k + 1
    m[:, :e] = 0
    m[:, -e:] = 0
    m[:, :, :e] = 0
    m[:, :, -e:] = 0
    return m
