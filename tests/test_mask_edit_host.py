"""CPU: the mask-edit calls exist at every layer (header, library, ctypes, class) and refuse bad
arguments without touching a device; the numpy reference the GPU tests compare against
(mask_edit_ref) is scipy.ndimage's binary morphology with the pads the header fixes; and the shared
inputs are such that no operation is trivial on them."""
import os
import re

import numpy as np
import pytest

from conftest import REPO
from vent_analysis_amd import _lib

import mask_edit_ref as M

NEW = ("vh_batch_edit_mask", "vh_batch_paint_mask", "vh_batch_download_mask", "vh_edit_mask")
NAMES = ("mask_stats;gather;sort;mean;classify;cohort;kmeans;snr;border;n4_init;n4_den;n4_hist;"
         "n4_fit;n4_contract;n4_eval;n4_welford;n4_pcw;n4_pcg;n4_final;n4_study;ci_walk;vdp_chain;"
         "ci_walk_b;defect_sel")


def test_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(REPO, "include", "vent_hip.h")).read()
    L = _lib.lib()
    for n in NEW:
        assert re.search(r"^int %s\(vh_(batch|ctx) \*" % n, hdr, re.M), n
        assert hasattr(L, n), n
        assert n in _lib._SIGS, n
    for name, val in (("VH_MASK_ERODE", 0), ("VH_MASK_DILATE", 1), ("VH_MASK_OPEN", 2), ("VH_MASK_CLOSE", 3),
                      ("VH_PAINT_OR", 0), ("VH_PAINT_ANDNOT", 1), ("VH_PAINT_AND", 2), ("VH_PAINT_XOR", 3)):
        assert re.search(r"^#define %s %d$" % (name, val), hdr, re.M), name
        assert getattr(_lib, name) == val
    assert "Vent_Analysis.py:1023" in hdr
    assert L.vh_batch_kernel_names().decode() == NAMES   # "mask_edit_b" is timed but not listed
    assert L.vh_abi_version() == 8   # additions only
    for n in ("edit_mask", "paint_mask", "download_mask"):
        assert callable(getattr(_lib.Batch, n)), n
    assert callable(_lib.edit_mask) and callable(_lib._mask_edit_args)
    from vent_analysis_amd import Vent_Analysis
    assert callable(Vent_Analysis.edit_mask)
    assert "calculate_VDP" in Vent_Analysis.edit_mask.__doc__ and "old mask" in Vent_Analysis.edit_mask.__doc__


def test_null_handles_are_argument_errors():
    """Checked before anything is dereferenced: no device is needed."""
    L = _lib.lib()
    buf = np.ones(64, np.uint8)
    rad = np.ones(4, np.int32)
    cnt = np.zeros(4, np.int64)
    p = _lib._ptr
    assert L.vh_batch_edit_mask(None, 0, p(rad)) == _lib.VH_ERR_ARG
    assert L.vh_batch_paint_mask(None, p(buf), 0) == _lib.VH_ERR_ARG
    assert L.vh_batch_download_mask(None, p(buf), p(cnt)) == _lib.VH_ERR_ARG
    assert L.vh_edit_mask(None, p(buf), 2, 2, 2, 1, 0, p(rad), p(buf), p(cnt)) == _lib.VH_ERR_ARG


@pytest.mark.parametrize("op,radius,n", [("erode", -1, 2), ("erode", 6, 2), ("erode", 2.5, 2),
                                         ("erode", [1, 2, 3], 2), ("erode", [1, 6], 2), ("erode", [1.0, 2.0], 2),
                                         ("erode", True, 2), ("erode", [[1, 2]], 2), ("grow", 1, 2), (4, 1, 2),
                                         (-1, 1, 2), (1.0, 1, 2), (None, 1, 2)], ids=str)
def test_argument_errors_are_value_errors(op, radius, n):
    """The checks of vh_batch_edit_mask, made by the binding first: ValueError, no device call."""
    with pytest.raises(ValueError):
        _lib._mask_edit_args(op, radius, n)


@pytest.mark.parametrize("how", ("paint", 4, -1, 1.0, None, True), ids=str)
def test_an_unknown_paint_mode_is_a_value_error(how):
    with pytest.raises(ValueError):
        _lib.paint_mode(how)


def test_argument_forms():
    for i, name in enumerate(M.OPS):
        assert _lib._mask_edit_args(name, 1, 1)[0] == i == _lib._mask_edit_args(np.int64(i), 1, 1)[0]
    for i, name in enumerate(M.HOWS):
        assert _lib.paint_mode(name) == i == _lib.paint_mode(np.int32(i))
    op, r = _lib._mask_edit_args("open", np.int64(5), 3)
    assert op == _lib.VH_MASK_OPEN and r.dtype == np.int32 and r.flags.c_contiguous and r.tolist() == [5, 5, 5]
    op, r = _lib._mask_edit_args(1, np.array([0, 5, 2], np.uint8), 3)
    assert op == _lib.VH_MASK_DILATE and r.dtype == np.int32 and r.tolist() == [0, 5, 2]
    assert _lib._mask_edit_args("close", (3, 0), 2)[1].tolist() == [3, 0]


# ---- the reference itself ------------------------------------------------------------------------
def test_the_disc_sizes():
    assert [len(M.disc(k)) for k in range(1, 6)] == [5, 13, 29, 49, 81]


def test_the_inputs_are_as_described():
    for shape in M.SHAPES:
        m = M.batch_masks(shape)
        assert m.dtype == np.uint8 and m.shape == (4,) + shape and not m.flags.writeable
        assert set(np.unique(m[0])) <= {0, 1} and set(np.unique(m[1])) <= {0, 2, 255}
        assert not m[2].any() and (m[3] == 1).all()
        assert m is M.batch_masks(shape)
    m = M.batch_masks((64, 64, 24))
    assert set(np.unique(m[1])) == {0, 2, 255}
    assert m[1][0].any() and m[1][:, -1].any()          # the mask touches row 0 and the last column
    st = M.batch_strokes((41, 37, 9))
    assert set(np.unique(st)) == {0, 7, 255} and st[0].reshape(-1)[-1] and st[1].reshape(-1)[0]


@pytest.mark.parametrize("shape", M.SHAPES, ids=str)
def test_the_reference_is_scipys_binary_morphology(shape):
    ndi = pytest.importorskip("scipy.ndimage")
    masks = M.batch_masks(shape)
    for k in range(1, 6):
        d = np.zeros((2 * k + 1, 2 * k + 1), bool)
        for dr, dc in M.disc(k):
            d[k + dr, k + dc] = True
        for q in range(4):
            s = masks[q] != 0
            dil, ero, ope, clo = M.dilate(s, k), M.erode(s, k), M.open_(s, k), M.close(s, k)
            assert np.array_equal(dil, ndi.binary_dilation(s, structure=d[:, :, None])), (k, q)
            assert np.array_equal(ero, ndi.binary_erosion(s, structure=d[:, :, None], border_value=1)), (k, q)
            assert not (ope & ~s).any() and not (s & ~clo).any(), (k, q)          # open in s in close
            assert np.array_equal(M.open_(ope, k), ope) and np.array_equal(M.close(clo, k), clo), (k, q)
            assert np.array_equal(ero, ~M.dilate(~s, k)), (k, q)                  # duality, pads swapped
            assert np.array_equal(dil, ~M.erode(~s, k)), (k, q)
        assert M.edit(masks[3], "open", k).all() and M.edit(masks[3], "erode", k).all()


def test_radius_zero_keeps_the_bytes_and_edit_writes_zero_one():
    m = M.batch_masks((41, 37, 9))
    assert np.array_equal(M.edit(m[1], "erode", 0), m[1]) and 255 in M.edit(m[1], "close", 0)
    for op in M.OPS:
        out = M.edit(m[1], op, 2)
        assert out.dtype == np.uint8 and set(np.unique(out)) == {0, 1}
    ref = M.batch_reference((41, 37, 9), "open", (3, 0, 3, 0))
    assert np.array_equal(ref[1], m[1]) and np.array_equal(ref[0], M.open_(m[0], 3))


def test_paint_truth_tables():
    mask = np.array([0, 0, 0, 2, 2, 2, 255, 255, 255], np.uint8).reshape(3, 3, 1)
    strokes = np.array([0, 7, 255, 0, 7, 255, 0, 7, 255], np.uint8).reshape(3, 3, 1)
    want = dict([("or", [0, 1, 1, 1, 1, 1, 1, 1, 1]), ("andnot", [0, 0, 0, 1, 0, 0, 1, 0, 0]),
                 ("and", [0, 0, 0, 0, 1, 1, 0, 1, 1]), ("xor", [0, 1, 1, 1, 0, 0, 1, 0, 0])])
    assert tuple(want) == M.HOWS
    for how in M.HOWS:
        out = M.paint(mask, strokes, how)
        assert out.dtype == np.uint8 and out.reshape(-1).tolist() == want[how], how


@pytest.mark.parametrize("shape", [(41, 37, 9), (64, 64, 24)], ids=str)
def test_no_operation_is_trivial_on_the_inputs(shape):
    """A condition on the inputs, checked with the reference alone: on studies 0 and 1 every op at
    every radius changes the mask and leaves it neither empty nor full, and for every radius some
    slice's result differs from slice 0's."""
    masks = M.batch_masks(shape)
    for q in (0, 1):
        s = masks[q] != 0
        for k in range(1, 6):
            for op in M.OPS:
                out = M.edit(masks[q], op, k).astype(bool)
                assert not np.array_equal(out, s), (q, op, k)
                assert out.any() and not out.all(), (q, op, k)
                assert any(not np.array_equal(out[:, :, z], out[:, :, 0]) for z in range(1, shape[2])), (q, op, k)
