"""CPU: the batch rendering calls exist at every layer (header, library, ctypes, Batch), refuse a
null batch without touching a device, the crops the GPU cases rely on are what cropToData gives, and
Batch.montage's slicing of the compact buffer is right."""
import os
import re

import numpy as np
import pytest

from conftest import REPO
from vent_analysis_amd import _lib

import batch_render_ref as BR

NEW = ("vh_batch_overlay", "vh_batch_download_overlay", "vh_batch_montage_layout", "vh_batch_montage",
       "vh_batch_download_montage")
KERNEL_NAMES = ("mask_stats;gather;sort;mean;classify;cohort;kmeans;snr;border;n4_init;n4_den;n4_hist;"
                "n4_fit;n4_contract;n4_eval;n4_welford;n4_pcw;n4_pcg;n4_final;n4_study;ci_walk;vdp_chain;"
                "ci_walk_b;defect_sel")


def test_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(REPO, "include", "vent_hip.h")).read()
    L = _lib.lib()
    for n in NEW:
        assert re.search(r"^int %s\(vh_batch \*" % n, hdr, re.M), n
        assert hasattr(L, n), n
        assert n in _lib._SIGS, n
    for m in ("overlay", "montage_layout", "montage"):
        assert callable(getattr(_lib.Batch, m, None)), m
    assert L.vh_abi_version() == 8   # additions only
    assert L.vh_batch_kernel_names().decode() == KERNEL_NAMES
    assert "overlay_b" in hdr and "montage_b" in hdr   # the two timing classes are named in the header


def test_null_batch_is_an_argument_error():
    """Checked before anything is dereferenced: no device is needed."""
    L = _lib.lib()
    buf = np.zeros(64, np.uint8)
    pal = np.zeros((4, 3), np.float64)
    p = _lib._ptr(buf)
    assert L.vh_batch_overlay(None) == _lib.VH_ERR_ARG
    assert L.vh_batch_download_overlay(None, p) == _lib.VH_ERR_ARG
    assert L.vh_batch_montage_layout(None, p, p, p) == _lib.VH_ERR_ARG
    assert L.vh_batch_montage(None, None, _lib._ptr(pal), 4) == _lib.VH_ERR_ARG
    assert L.vh_batch_download_montage(None, p, p) == _lib.VH_ERR_ARG


@pytest.mark.parametrize("shape,mask,crop", [
    ((41, 37, 9), BR.ellipse, (4, 34, 5, 28, 1, 7)),
    ((41, 37, 9), BR.block, (0, 25, 0, 17, 1, 1)),
    ((41, 37, 9), BR.corner, (33, 8, 30, 7, 8, 1)),
    ((19, 70, 5), BR.ellipse, (0, 19, 13, 45, 1, 3)),
    ((19, 70, 5), BR.block, (0, 14, 0, 28, 1, 1)),
    ((19, 70, 5), BR.wide, (0, 19, 0, 70, 1, 3)),          # 64 + 6 columns
    ((24, 20, 70), BR.ellipse, (0, 24, 0, 20, 1, 68)),     # 32 + 32 + 4 slices
    ((128, 128, 24), BR.ellipse, (21, 87, 27, 75, 1, 22)),  # 64 + 11 columns
], ids=lambda v: getattr(v, "__name__", None) or "_".join(map(str, v)))   # no address in an id
def test_reference_crops(shape, mask, crop):
    """Drift in the inputs of the GPU cases is noticed."""
    assert BR.crop6(mask(shape)) == crop
    assert BR.crop6(mask(shape) * np.uint8(255)) == crop   # sum > 0, whatever the mask's value


@pytest.mark.parametrize("mask", [BR.row0, BR.slice0, lambda s: np.zeros(s, np.uint8)],
                         ids=["row0", "slice0", "empty"])
def test_reference_raises_on_index0_and_empty(mask):
    with pytest.raises(IndexError):
        BR.crop6(mask((41, 37, 9)))


def test_expected_layout_of_the_mixed_batch():
    hp, mk, proton = BR.mixed_batch()
    crop, status = BR.expected_layout(mk)
    assert list(status) == [0, 0, 0, BR.VH_ERR_EMPTY, BR.VH_ERR_EMPTY, 0, 0]
    assert tuple(crop[0]) == tuple(crop[5]) == tuple(crop[6]) == (4, 34, 5, 28, 1, 7)
    assert not crop[3].any() and not crop[4].any()
    assert (BR.VH_OK, BR.VH_ERR_EMPTY, BR.VH_ERR_INDEX) == (_lib.VH_OK, _lib.VH_ERR_EMPTY, _lib.VH_ERR_INDEX)


def test_montage_views_slice_the_compact_buffer():
    """A hand-made buffer: three studies, the middle one without an image, starts aligned to 64."""
    crop = np.array([[2, 3, 1, 4, 0, 2], [0, 0, 0, 0, 0, 0], [0, 1, 0, 5, 3, 1]], np.int64)
    n0, n2 = 21 * 3 * 4 * 2, 21 * 1 * 5 * 1
    off = np.array([0, 512, 512, 640], np.int64)   # n0 = 504 -> 512
    status = np.array([_lib.VH_OK, _lib.VH_ERR_EMPTY, _lib.VH_OK], np.int32)
    buf = (np.arange(640) % 251).astype(np.uint8)
    v = _lib.montage_views(buf, crop, off, status)
    assert v[1] is None
    assert v[0].shape == (21, 8, 3) and v[2].shape == (7, 5, 3)
    assert np.array_equal(v[0].ravel(), buf[:n0]) and np.array_equal(v[2].ravel(), buf[512:512 + n2])
    assert v[0][20, 7, 2] == buf[n0 - 1] and v[2][1, 0, 0] == buf[512 + 15]   # row-major [row][x][rgb]
    assert np.shares_memory(v[0], buf)   # views
    status[2] = _lib.VH_ERR_INDEX
    assert _lib.montage_views(buf, crop, off, status)[2] is None
    with pytest.raises(ValueError):   # an image past the buffer's end
        _lib.montage_views(buf[:600], crop, off, np.zeros(3, np.int32))
