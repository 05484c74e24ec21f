"""GPU: the lungs from the proton image of a resident batch (vh_batch_upload_proton /
vh_batch_proton_threshold / vh_batch_segment / vh_batch_mask_overlap and the layers above them)
against the numpy reference (segment_ref).  Every step is a max, an integer count or bit logic: the
comparisons are np.array_equal on uint8 and == on float32."""
import functools

import numpy as np
import pytest

from vent_analysis_amd import _lib

import mask_edit_ref as M
import segment_ref as S

pytestmark = pytest.mark.gpu

VOX = (1.5, 1.5, 10.0)


def same_bytes(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == np.uint8 and a.shape == b.shape and np.array_equal(a, b)


def studies(shape):
    return 2 if shape == S.BIG else 4


@functools.lru_cache(maxsize=None)
def resident(shape):
    """One batch per shape with its proton uploaded, kept for the parametrised cases."""
    n = studies(shape)
    B = _lib.Batch(*shape, n)
    B.upload_proton(S.batch_proton(shape)[:n])
    return B


@functools.lru_cache(maxsize=None)
def volumes(shape, n=4):
    rng = np.random.default_rng(13)
    hp = (rng.random((n,) + tuple(shape), dtype=np.float32) * 100 + 5).astype(np.float32)
    hp.setflags(write=False)
    return hp


@pytest.mark.parametrize("shape", S.SHAPES + [S.BIG], ids=str)
def test_proton_threshold_equals_the_reference(shape):
    n = studies(shape)
    th, pmax, hist = resident(shape).proton_threshold(stats=True)
    rt, rp, rh = S.batch_stats(shape, n)
    assert pmax.dtype == np.float32 and np.array_equal(pmax, rp), (pmax, rp)
    assert hist.dtype == np.uint32 and hist.shape == (n, 256)
    for q in range(n):
        assert np.array_equal(hist[q], rh[q]), (q, np.flatnonzero(hist[q] != rh[q])[:8])
    assert th.dtype == np.float32 and (th == rt).all(), (th, rt)
    assert np.array_equal(resident(shape).proton_threshold(), rt)       # the sweep starts from zeroed counters


def test_a_study_without_a_threshold_is_nan():
    shape = (41, 37, 9)
    x = S.batch_proton(shape).copy()
    x[1] = 0.0                            # all zero: pmax is not > 0
    x[2] = np.float32(7.5)                # one occupied bin
    x[3] = np.where(x[3] > 50, np.nan, -1.0)   # F is empty
    B = _lib.Batch(*shape, 4)
    B.upload_proton(x)
    th, pmax, hist = B.proton_threshold(stats=True)
    assert th[0] == S.batch_stats(shape)[0][0] and np.isnan(th[1:]).all()
    assert pmax.tolist()[1:] == [0.0, 7.5, 0.0]
    assert not hist[1].any() and not hist[3].any() and hist[2][255] == x[2].size and hist[2].sum() == x[2].size
    B.upload(None, M.batch_masks(shape))
    with pytest.raises(ValueError, match=r"\[1, 2, 3\]"):
        B.segment()
    assert same_bytes(B.download_mask(), M.batch_masks(shape))           # nothing was enqueued
    with pytest.raises(IndexError):
        _lib.segment(x)
    B.close()


WIDTHS = [(shape, zc) for shape in S.SHAPES + [S.BIG] for zc in (None,) + S.ZCS
          if zc is None or S.zc_fits(shape, zc)]


@pytest.mark.parametrize("shape,zc", WIDTHS, ids=lambda v: str(v).replace(" ", ""))
def test_segment_equals_the_reference(shape, zc, monkeypatch):
    """Byte for byte, for every packing width that fits the plane (VH_SEG_ZC is read at call time; unset,
    the library chooses), every set of radii, and the voxel counts."""
    if zc is None:
        monkeypatch.delenv("VH_SEG_ZC", raising=False)
    else:
        monkeypatch.setenv("VH_SEG_ZC", str(zc))
    n = studies(shape)
    B = resident(shape)
    for radii in S.RADII:
        used = B.segment(S.THRESH[:n], radii[:n])
        got, cnt = B.download_mask(count=True)
        ref = S.batch_reference(shape, radii[:n], False, n)
        assert used.dtype == np.float32 and used.tolist() == list(S.THRESH[:n])
        for q in range(n):
            assert same_bytes(got[q], ref[q]), (radii, q, int((got[q] != ref[q]).sum()), np.argwhere(got[q] != ref[q])[:4])
        assert cnt.dtype == np.int64 and cnt.tolist() == [int(ref[q].sum()) for q in range(n)]


@pytest.mark.parametrize("shape", S.SHAPES, ids=str)
def test_the_otsu_default(shape):
    B = resident(shape)
    used = B.segment(open_radius=(1, 0, 0, 2))
    assert np.array_equal(used, S.batch_stats(shape)[0])
    assert same_bytes(B.download_mask(), S.batch_reference(shape, (1, 0, 0, 2), True))


def test_segment_puts_the_batch_back_to_uploaded_and_the_next_run_sees_the_mask():
    shape = (41, 37, 9)
    hp, masks = volumes(shape), M.batch_masks(shape)
    from vent_analysis_amd.sphere import compact_table_for
    defect = (np.random.default_rng(7).random((4,) + shape) < 0.2).astype(np.uint8)
    table = compact_table_for(VOX, 12, shape)     # a small sphere table: 12 mm
    B = _lib.Batch(*shape, 4)
    B.upload(hp, masks)
    B.upload_defect(defect)
    B.ci(VOX, table=table)
    ci_before = B.download_ci()
    B.upload_proton(S.batch_proton(shape))
    B.run(B.options(do_n4=False, vox=VOX))
    B.download()
    B.upload_defect(defect)
    B.segment(S.THRESH, (1, 2, 0, 5))
    ref = S.batch_reference(shape, (1, 2, 0, 5))
    for call in (B.download, lambda: B.select_defect("mean"), B.distribution, B.overlay, B.montage_layout,
                 B.km_cuts):
        with pytest.raises(ValueError):
            call()
    assert np.array_equal(B.download_hp(), hp)                            # HPvent survives
    B.ci(VOX, table=table)                                                # ... and a set_defect map
    for a, b in zip(ci_before, B.download_ci()):
        assert np.array_equal(a, b, equal_nan=True)
    B.edit_mask("dilate", (1, 0, 2, 0))                                   # edit_mask composes
    ref2 = M.batch_edit(ref, "dilate", (1, 0, 2, 0))
    ref2[2] = 1                                                           # (study 2 is empty: run on a full mask)
    B.paint_mask(np.stack([np.zeros(shape, np.uint8)] * 2 + [np.ones(shape, np.uint8)] + [np.zeros(shape, np.uint8)]))
    B.run(B.options(do_n4=False, vox=VOX))
    res = B.download()[4]
    got, cnt = B.download_mask(count=True)
    B.close()
    assert same_bytes(got, ref2)
    assert [r.n_mask for r in res] == cnt.tolist() == ref2.reshape(4, -1).sum(axis=1).tolist()


@pytest.mark.parametrize("shape", [(41, 37, 9), (64, 64, 24)], ids=str)
def test_mask_overlap(shape):
    """A 0/2/255 other mask; at (41, 37, 9) V is no multiple of 16, so studies start off a 16-byte word."""
    other = M.batch_masks(shape)
    assert set(np.unique(other[1])) == {0, 2, 255} and (shape != (41, 37, 9) or other[0].size % 16)
    B = resident(shape)
    B.segment(S.THRESH, 0)
    seg = S.batch_reference(shape, (0, 0, 0, 0))
    want = [[int(seg[q].sum()), int((other[q] != 0).sum()), int(((seg[q] != 0) & (other[q] != 0)).sum())]
            for q in range(4)]
    got = B.mask_overlap(other)
    assert got.dtype == np.int64 and got.tolist() == want
    assert B.mask_overlap(other.astype(np.float64)).tolist() == want
    assert B.mask_overlap(seg)[:, 2].tolist() == [w[0] for w in want]      # with itself
    assert same_bytes(B.download_mask(), seg)                              # the resident mask is only read


def test_host_buffer_form_and_class_method():
    from vent_analysis_amd import Vent_Analysis
    shape = (64, 64, 24)
    x = S.batch_proton(shape)
    got, used, cnt = _lib.segment(x, S.THRESH, (1, 2, 0, 5), count=True)
    ref = S.batch_reference(shape, (1, 2, 0, 5))
    assert same_bytes(got, ref) and used.tolist() == list(S.THRESH) and cnt.tolist() == ref.reshape(4, -1).sum(1).tolist()
    got, used = _lib.segment(x.astype(np.float64), open_radius=(1, 0, 0, 2))
    assert same_bytes(got, S.batch_reference(shape, (1, 0, 0, 2), True)) and np.array_equal(used, S.batch_stats(shape)[0])
    one, t1 = _lib.segment(x[0], 40.0, 1)                                  # a 3-D volume, scalars
    assert same_bytes(one[0], S.batch_reference(shape, (1, 1, 1, 1))[0]) and t1.tolist() == [40.0]
    va = Vent_Analysis(pickle_dict=dict(HPvent=volumes(shape)[0].copy(), mask=M.batch_masks(shape)[1].astype(np.float64),
                                        vox=list(VOX)))
    with pytest.raises(ValueError):
        va.segment_mask()                                                  # no proton
    va.proton = x[0].astype(np.float64)
    out = va.segment_mask()
    ref0 = S.batch_reference(shape, (1, 0, 0, 2), True)[0]
    assert out is va.mask and out.dtype == np.float64 and np.array_equal(out, ref0.astype(np.float64))
    assert np.array_equal(va.mask_border, va.calculateBorder(ref0))
    assert va.metadata["LungVolume"] == np.sum(ref0 == 1) * np.prod(np.divide(list(VOX), 10)) / 1000
    assert np.array_equal(va.segment_mask(40.0, 0), S.batch_reference(shape, (0, 0, 0, 0))[0].astype(np.float64))
    for bad in (dict(thresh=np.nan), dict(thresh=0.0), dict(open_radius=6)):
        with pytest.raises(ValueError):
            va.segment_mask(**bad)
    va.proton = x[0][:-1]
    with pytest.raises(ValueError):
        va.segment_mask()


def test_library_argument_errors():
    """The library's own checks (the binding's are bypassed): VH_ERR_ARG, nothing enqueued -- the mask is
    unchanged afterwards."""
    shape = (41, 37, 9)
    masks = M.batch_masks(shape)
    p = _lib._ptr
    B = _lib.Batch(*shape, 4)
    B.upload(None, masks)
    ok_t, ok_r = np.array(S.THRESH, np.float32), np.array([1, 2, 0, 1], np.int32)
    th = np.zeros(4, np.float32)
    assert B.L.vh_batch_segment(B.h, p(ok_t), p(ok_r)) == _lib.VH_ERR_ARG             # no proton
    assert B.L.vh_batch_proton_threshold(B.h, p(th), None, None) == _lib.VH_ERR_ARG
    with pytest.raises(ValueError):
        B.segment(40.0)
    with pytest.raises(ValueError):
        B.segment()
    B.upload_proton(S.batch_proton(shape))
    for t, r in ((None, ok_r), (np.array([40, np.nan, 4, 50], np.float32), ok_r),
                 (np.array([40, 0.5, 0, 50], np.float32), ok_r), (np.array([40, 0.5, 4, -1], np.float32), ok_r),
                 (np.array([np.inf, 0.5, 4, 50], np.float32), ok_r), (ok_t, np.array([1, 2, 6, 1], np.int32)),
                 (ok_t, np.array([-1, 2, 0, 1], np.int32))):
        assert B.L.vh_batch_segment(B.h, p(t), p(r)) == _lib.VH_ERR_ARG, (t, r)
    assert B.L.vh_batch_upload_proton(B.h, None) == _lib.VH_ERR_ARG
    assert B.L.vh_batch_proton_threshold(B.h, None, None, None) == _lib.VH_ERR_ARG
    cnt = np.zeros((4, 3), np.int64)
    assert B.L.vh_batch_mask_overlap(B.h, None, p(cnt)) == _lib.VH_ERR_ARG
    assert B.L.vh_batch_mask_overlap(B.h, p(np.ascontiguousarray(masks)), None) == _lib.VH_ERR_ARG
    for bad in (dict(thresh=np.nan), dict(thresh=0.0), dict(thresh=-2.0), dict(thresh=1.0, open_radius=6)):
        with pytest.raises(ValueError):
            B.segment(**bad)
    assert same_bytes(B.download_mask(), masks)
    assert B.L.vh_batch_segment(B.h, p(ok_t), None) == _lib.VH_OK                     # NULL radii: no opening
    assert same_bytes(B.download_mask(), S.batch_reference(shape, (0, 0, 0, 0)))
    B.close()
    # a plane of 513 columns: the library refuses it, and so does the binding before any device call
    wide = (4, 513, 2)
    W = _lib.Batch(*wide, 1)
    m = np.ones((1,) + wide, np.uint8)
    x = np.ones((1,) + wide, np.float32)
    W.upload(None, m)
    W.upload_proton(x)
    one = np.array([0.5], np.float32)
    assert W.L.vh_batch_segment(W.h, p(one), None) == _lib.VH_ERR_ARG
    with pytest.raises(ValueError):
        W.segment(0.5)
    assert same_bytes(W.download_mask(), m)
    c = W.ctx
    out = np.empty_like(m)
    assert c.L.vh_segment(c.h, p(x), 4, 513, 2, 1, p(one), None, p(out), None, None) == _lib.VH_ERR_ARG
    assert c.L.vh_segment(c.h, None, 4, 8, 2, 1, p(one), None, p(out), None, None) == _lib.VH_ERR_ARG
    with pytest.raises(ValueError):
        _lib.segment(x, 0.5)
    W.close()
