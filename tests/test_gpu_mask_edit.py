"""GPU: editing the masks of a resident batch (vh_batch_edit_mask / vh_batch_paint_mask /
vh_batch_download_mask and the layers above them) against the numpy reference (mask_edit_ref).  All
arithmetic is on bits: every comparison is np.array_equal on uint8."""
import ctypes as ct
import functools

import numpy as np
import pytest

from vent_analysis_amd import _lib

import mask_edit_ref as M

pytestmark = pytest.mark.gpu

VOX = (1.5, 1.5, 10.0)


def same_bytes(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == np.uint8 and a.shape == b.shape and np.array_equal(a, b)


@functools.lru_cache(maxsize=None)
def resident(shape):
    """One batch of four studies per shape, kept for the parametrised cases (each uploads again: an
    edit replaces the resident mask)."""
    return _lib.Batch(*shape, 4)


@functools.lru_cache(maxsize=None)
def volumes(shape, n=4):
    rng = np.random.default_rng(11)
    hp = (rng.random((n,) + tuple(shape), dtype=np.float32) * 100 + 5).astype(np.float32)
    hp *= 0.25 + (M.batch_masks(shape)[:n] != 0)      # signal inside the mask, background outside
    hp.setflags(write=False)
    return hp


@pytest.mark.parametrize("radii", M.RADII, ids=str)
@pytest.mark.parametrize("op", M.OPS)
@pytest.mark.parametrize("shape", M.SHAPES, ids=str)
def test_edit_mask_equals_the_reference(shape, op, radii):
    masks = M.batch_masks(shape)
    B = resident(shape)
    B.upload(None, masks)
    used = B.edit_mask(op, radii)
    got, cnt = B.download_mask(count=True)
    ref = M.batch_reference(shape, op, radii)
    assert used.tolist() == list(radii)
    for q in range(4):
        assert same_bytes(got[q], ref[q]), (q, int((got[q] != ref[q]).sum()), np.argwhere(got[q] != ref[q])[:4])
    assert cnt.dtype == np.int64 and cnt.tolist() == [int((ref[q] != 0).sum()) for q in range(4)]
    assert not got[2].any() and (got[3] == 1).all()
    if radii[1] == 0:
        assert same_bytes(got[1], masks[1]) and 255 in got[1] and 2 in got[1]   # byte for byte


@pytest.mark.parametrize("op", M.OPS)
@pytest.mark.parametrize("shape", [(37, 70, 8), (9, 131, 32), (34, 66, 4)], ids=str)
def test_slices_that_pack_as_whole_words(shape, op):
    """When Z is a multiple of 4 up to 32 the kernel reads and writes a pixel as 32-bit words (of
    mask_edit_ref.SHAPES only (64, 64, 24) goes that way, in whole tiles): here with row and column
    remainders, a second column tile of two or three pixels, and a full 32-slice word."""
    masks = M.batch_masks(shape)
    B = resident(shape)
    for radii in ((5, 1, 4, 2), (3, 0, 3, 0)):
        B.upload(None, masks)
        B.edit_mask(op, radii)
        got, cnt = B.download_mask(count=True)
        ref = M.batch_reference(shape, op, radii)
        for q in range(4):
            assert same_bytes(got[q], ref[q]), (radii, q, int((got[q] != ref[q]).sum()))
        assert cnt.tolist() == [int((ref[q] != 0).sum()) for q in range(4)]


def test_two_edits_compose():
    """The output becomes the resident mask: a second call reads it."""
    shape = (41, 37, 9)
    B = resident(shape)
    B.upload(None, M.batch_masks(shape))
    B.edit_mask("open", (2, 1, 3, 1))
    B.edit_mask("dilate", (1, 3, 0, 2))
    got = B.download_mask()
    ref = M.batch_edit(M.batch_reference(shape, "open", (2, 1, 3, 1)), "dilate", (1, 3, 0, 2))
    assert same_bytes(got, ref)


@pytest.mark.parametrize("how", M.HOWS)
@pytest.mark.parametrize("shape", [(41, 37, 9), (33, 40, 33)], ids=str)
def test_paint(shape, how):
    """Strokes in {0, 7, 255} that cross a study boundary of the flat buffer (and, at these shapes, end
    in a byte tail); 0 / 1 bytes come back for every study, the 0/2/255 one included."""
    masks, strokes = M.batch_masks(shape), M.batch_strokes(shape)
    B = resident(shape)
    B.upload(None, masks)
    B.paint_mask(strokes, how)
    got, cnt = B.download_mask(count=True)
    ref = np.stack([M.paint(masks[q], strokes[q], how) for q in range(4)])
    assert same_bytes(got, ref) and set(np.unique(got)) == {0, 1}
    assert cnt.tolist() == ref.reshape(4, -1).sum(axis=1).tolist()


def test_download_mask_returns_the_resident_bytes():
    shape = (41, 37, 9)
    masks, hp = M.batch_masks(shape), volumes(shape)
    B = _lib.Batch(*shape, 4)
    B.upload(hp, masks)
    got, cnt = B.download_mask(count=True)
    assert same_bytes(got, masks) and cnt.tolist() == (masks != 0).reshape(4, -1).sum(axis=1).tolist()
    assert same_bytes(B.download_mask(), masks)
    B.run(B.options(do_n4=False, vox=VOX))
    assert same_bytes(B.download_mask(), masks)       # after a run it still does
    B.download()                                      # ... and the run's results are still there
    B.close()


def result_bytes(res):
    return [bytes(r) for r in res]


@functools.lru_cache(maxsize=None)
def downstream(do_n4):
    """(41, 37, 9), studies 0 and 1: (a) upload, erode by 1, run, download; (b) a fresh batch uploaded
    with the reference-eroded mask, run, download."""
    shape = (41, 37, 9)
    hp, masks = volumes(shape)[:2], M.batch_masks(shape)[:2]
    ref = M.batch_reference(shape, "erode", (1, 1, 1, 1))[:2]
    out = []
    for src, ed in ((masks, True), (ref, False)):
        B = _lib.Batch(*shape, 2)
        B.upload(hp, src)
        if ed:
            B.edit_mask("erode", 1)
        B.run(B.options(do_n4=do_n4, vox=VOX))
        r = B.download(n4=True)
        B.distribution("p99", 64, 1.5)
        out.append(r + (B.download_mask(), B.montage_layout(), B.download_distribution()))
        B.close()
    return out, ref


@pytest.mark.parametrize("do_n4", (False, True), ids=("plain", "n4"))
def test_the_next_run_sees_the_edited_mask(do_n4):
    """The mask statistics, N4 (when on), SNR and the VDP chain read the edited mask: every volume, map
    and scalar equals that of a fresh batch uploaded with the reference-eroded mask, and so do the
    montage layout and the distribution."""
    (a, b), ref = downstream(do_n4)
    assert same_bytes(a[5], ref) and same_bytes(b[5], ref)
    assert a[0].dtype == np.float32 and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    for k in (1, 2, 3):
        assert np.array_equal(a[k], b[k]), k
    assert result_bytes(a[4]) == result_bytes(b[4])
    assert a[4][0].n_mask == int(ref[0].sum()) and a[4][1].n_mask == int(ref[1].sum())
    for x, y in zip(a[6], b[6]):
        assert np.array_equal(x, y)
    assert set(a[7]) == set(b[7])
    for key in a[7]:
        assert np.array_equal(a[7][key], b[7][key]), key


@pytest.mark.parametrize("edit", ("morphology", "paint"))
def test_after_a_run_an_edit_puts_the_batch_back_to_uploaded(edit):
    shape = (41, 37, 9)
    hp, masks = volumes(shape), M.batch_masks(shape)
    B = _lib.Batch(*shape, 4)
    B.upload(hp, masks)
    B.run(B.options(do_n4=False, vox=VOX))
    B.download()
    if edit == "paint":
        B.paint_mask(M.batch_strokes(shape), "andnot")
        ref = np.stack([M.paint(masks[q], M.batch_strokes(shape)[q], "andnot") for q in range(4)])
    else:
        B.edit_mask("close", 2)
        ref = M.batch_reference(shape, "close", (2, 2, 2, 2))
    for call in (B.download, B.download_defect, lambda: B.select_defect("mean"), B.distribution, B.overlay,
                 B.montage_layout, B.km_cuts):
        with pytest.raises(ValueError):
            call()
    B.run(B.options(do_n4=False, vox=VOX))
    res = B.download()[4]
    got = B.download_mask()
    B.close()
    assert same_bytes(got, ref)
    assert [r.n_mask for r in res] == ref.reshape(4, -1).sum(axis=1).tolist()


def test_a_map_from_set_defect_survives_an_edit():
    from vent_analysis_amd.sphere import compact_table_for
    shape = (41, 37, 9)
    masks = M.batch_masks(shape)
    defect = (np.random.default_rng(7).random((4,) + shape) < 0.2).astype(np.uint8)
    table = compact_table_for(VOX, 12, shape)     # a small sphere table: 12 mm
    out = []
    for ed in (False, True):
        B = _lib.Batch(*shape, 4)
        B.upload(volumes(shape), masks)
        B.upload_defect(defect)
        if ed:
            B.edit_mask("open", (2, 5, 1, 3))
            B.paint_mask(M.batch_strokes(shape), "xor")
        B.ci(VOX, table=table)
        out.append(B.download_ci())
        B.close()
    (m0, s0, st0), (m1, s1, st1) = out
    assert np.array_equal(m0, m1) and np.array_equal(st0, st1)
    assert np.array_equal(s0, s1, equal_nan=True) and (m0 >= 0).any()


def test_library_argument_errors():
    """The library's own checks (the binding's are bypassed): VH_ERR_ARG, nothing enqueued."""
    shape = (5, 7, 3)
    masks = M.batch_masks(shape)
    B = resident(shape)
    B.upload(None, masks)
    ok = np.array([1, 2, 0, 1], np.int32)
    strokes = np.ascontiguousarray(M.batch_strokes(shape))
    edit = lambda op, r: B.L.vh_batch_edit_mask(B.h, op, _lib._ptr(r))  # noqa: E731
    for op, r in ((0, None), (-1, ok), (4, ok), (0, np.array([1, -1, 0, 1], np.int32)),
                  (3, np.array([1, 2, 6, 1], np.int32))):
        assert edit(op, r) == _lib.VH_ERR_ARG, (op, r)
    assert B.L.vh_batch_paint_mask(B.h, _lib._ptr(strokes), 4) == _lib.VH_ERR_ARG
    assert B.L.vh_batch_paint_mask(B.h, _lib._ptr(strokes), -1) == _lib.VH_ERR_ARG
    assert B.L.vh_batch_paint_mask(B.h, None, 0) == _lib.VH_ERR_ARG
    with pytest.raises(ValueError):
        B.ctx.check(edit(4, ok), "vh_batch_edit_mask")
    c = B.ctx
    m = np.ascontiguousarray(masks)
    out = np.empty_like(m)
    assert c.L.vh_edit_mask(c.h, _lib._ptr(m), 5, 7, 3, 4, 0, None, _lib._ptr(out), None) == _lib.VH_ERR_ARG
    assert c.L.vh_edit_mask(c.h, _lib._ptr(m), 5, 7, 3, 4, 7, _lib._ptr(ok), _lib._ptr(out), None) == _lib.VH_ERR_ARG
    assert c.L.vh_edit_mask(c.h, None, 5, 7, 3, 4, 0, _lib._ptr(ok), _lib._ptr(out), None) == _lib.VH_ERR_ARG
    assert same_bytes(B.download_mask(), masks)       # the mask is unchanged
    assert edit(ct.c_int(2), ok) == _lib.VH_OK


def test_host_buffer_form_and_class_method():
    """vh_edit_mask on host arrays of any dtype and Vent_Analysis.edit_mask return the batch's bytes;
    the class method sets mask, mask_border and LungVolume and nothing else."""
    from vent_analysis_amd import Vent_Analysis
    shape = (64, 64, 24)
    masks = M.batch_masks(shape)
    got = _lib.edit_mask(masks.astype(np.float64), "close", (5, 1, 4, 2))
    assert same_bytes(got, M.batch_edit((masks != 0).astype(np.uint8), "close", (5, 1, 4, 2)))
    assert same_bytes(_lib.edit_mask(masks, "close", (3, 0, 3, 0)), M.batch_reference(shape, "close", (3, 0, 3, 0)))
    one = _lib.edit_mask(masks[0].astype(np.float64), "open", 3)          # a 3-D volume, a scalar radius
    assert same_bytes(one[0], M.edit(masks[0], "open", 3))
    va = Vent_Analysis(pickle_dict=dict(HPvent=volumes(shape)[0].copy(), mask=masks[1].astype(np.float64),
                                        vox=list(VOX)))
    before = {k: (v.copy() if isinstance(v, (np.ndarray, dict)) else v) for k, v in vars(va).items()}
    out = va.edit_mask("erode", 2)
    ref = M.edit(masks[1], "erode", 2)
    assert out is va.mask and out.dtype == np.float64 and np.array_equal(out, ref.astype(np.float64))
    assert set(np.unique(out)) == {0.0, 1.0}
    assert np.array_equal(va.mask_border, va.calculateBorder(ref))
    assert va.metadata["LungVolume"] == np.sum(ref == 1) * np.prod(np.divide(list(VOX), 10)) / 1000
    assert set(vars(va)) == set(before) | {"mask_border"}   # (a pickle holds no border: it is new here)
    for k, v in vars(va).items():
        if k == "metadata":
            assert {a: b for a, b in v.items() if a != "LungVolume"} == \
                {a: b for a, b in before[k].items() if a != "LungVolume"}
        elif k not in ("mask", "mask_border"):
            np.testing.assert_equal(v, before[k])
    strokes = M.batch_strokes(shape)[0]
    painted = va.edit_mask(strokes=strokes, how="xor")
    assert np.array_equal(painted, M.paint(ref, strokes, "xor").astype(np.float64))
    both = va.edit_mask("dilate", 1, strokes=strokes, how="andnot")
    assert np.array_equal(both, M.edit(M.paint(painted, strokes, "andnot"), "dilate", 1).astype(np.float64))
    with pytest.raises(ValueError):
        va.edit_mask()
    with pytest.raises(ValueError):
        va.edit_mask("erode", 6)
