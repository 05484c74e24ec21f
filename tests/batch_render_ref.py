"""Inputs and the CPU reference of the batch rendering tests (test_batch_render_host.py,
test_gpu_batch_render.py): the masks whose crops the tests pin, the fields, and cropToData /
screenShot / exportDICOM from oracle.export_oracle.  Not a test module."""
import functools
import os

import numpy as np

from oracle import export_oracle as E, vdp_oracle as O

from defect_select_ref import field

VOX = (1.5, 1.5, 10.0)
VH_OK, VH_ERR_EMPTY, VH_ERR_INDEX = 0, 5, 8
SMALL = (41, 37, 9)


def parula():
    """The reference's own 64 x 3 colour table (tests/golden/parula.npy)."""
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "parula.npy"), allow_pickle=False)


def ellipse(shape, scale=1.0, slices=None):
    """Centred ellipse, semi-axes 0.3 R and 0.25 C (times scale), on slices 1 .. Z - 2."""
    R, C, Z = shape
    i, j = np.meshgrid(np.arange(R), np.arange(C), indexing="ij")
    e = ((i - R / 2) / (0.3 * R * scale)) ** 2 + ((j - C / 2) / (0.25 * C * scale)) ** 2 <= 1
    m = np.zeros(shape, np.uint8)
    lo, hi = slices if slices is not None else (1, Z - 1)
    m[:, :, lo:hi] = e[:, :, None]
    return m


def block(shape):
    R, C, Z = shape
    m = np.zeros(shape, np.uint8)
    m[0:R // 2, 0:C // 3, 0:2] = 1
    return m


def corner(shape):
    R, C, Z = shape
    m = np.zeros(shape, np.uint8)
    m[R - 3:, C - 2:, Z - 1] = 1
    return m


def row0(shape):
    m = np.zeros(shape, np.uint8)
    m[0, 3:9, 1:4] = 1
    return m


def slice0(shape):
    m = np.zeros(shape, np.uint8)
    m[5:12, 3:9, 0] = 1
    return m


def wide(shape):
    """All but two columns on each side, slices 1 .. Z - 2: a crop wider than 64 columns at C = 70."""
    R, C, Z = shape
    m = np.zeros(shape, np.uint8)
    m[:, 2:C - 2, 1:Z - 1] = 1
    return m


def crop6(mask):
    """(r0, nr, c0, nc, s0, ns) of cropToData(mask, border=5); IndexError where the reference raises."""
    rr, cc, ss = E.crop_to_data(np.asarray(mask), border=5)
    return (rr[0], len(rr), cc[0], len(cc), ss[0], len(ss))


def expected_layout(mk):
    """(crop [B][6], status [B]) as vh_batch_montage_layout reports them."""
    crop = np.zeros((mk.shape[0], 6), np.int64)
    status = np.zeros(mk.shape[0], np.int32)
    for q in range(mk.shape[0]):
        try:
            crop[q] = crop6(mk[q])
        except IndexError:
            status[q] = VH_ERR_EMPTY
    return crop, status


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """Seven studies at 41 x 37 x 9: ellipse, block at the origin, corner block, a mask only in row 0,
    an empty mask, a constant HPvent 2.0 (normalize returns x itself: uint8(510) wraps) and the
    ellipse as a 0/255 mask.  (hp, mask, proton)."""
    s = SMALL
    hp = np.stack([field(s, 10 + q)[0] for q in range(7)])
    hp[5] = 2.0
    mk = np.stack([ellipse(s), block(s), corner(s), row0(s), np.zeros(s, np.uint8), ellipse(s),
                   ellipse(s) * np.uint8(255)])
    proton = np.stack([field(s, 30 + q)[0] for q in range(7)]) * np.float32(3.5) - np.float32(0.25)
    return _freeze(hp, mk, proton.astype(np.float32))


@functools.lru_cache(maxsize=None)
def shape_batch(shape):
    """Three studies of a shape (two at 128 x 128 x 24).  (hp, mask, proton)."""
    if shape == (128, 128, 24):
        masks = [ellipse(shape), block(shape)]
    elif shape == (19, 70, 5):
        masks = [ellipse(shape), block(shape), wide(shape)]
    else:
        masks = [ellipse(shape), block(shape), corner(shape)]
    n = len(masks)
    hp = np.stack([field(shape, 50 + q)[0] for q in range(n)])
    proton = np.stack([field(shape, 60 + q)[0] for q in range(n)])
    return _freeze(hp, np.stack(masks), proton)


@functools.lru_cache(maxsize=None)
def n4_batch():
    """Ellipse masks of three sizes at 41 x 37 x 9 for the run with N4 on."""
    s = SMALL
    hp = np.stack([field(s, 70 + q)[0] for q in range(3)])
    mk = np.stack([ellipse(s), ellipse(s, 0.7), ellipse(s, 1.3)])
    return _freeze(hp, mk)


def montage_ref(proton, hp, n4, mask, defect, ci, pal):
    """screenShot's array of one study; proton None = the zeros the class substitutes."""
    p = np.zeros_like(hp) if proton is None else np.asarray(proton, np.float32)
    return E.screenshot_image(p, hp, n4, mask, O.calculate_border(mask), defect, ci, pal)


def overlay_ref(n4, defect):
    return E.overlay_rgb(n4, defect)
