"""GPU: the proton resampled from its own grid onto the xenon grid of a resident batch
(vh_batch_upload_proton_src / vh_batch_resample_proton and the layers above them) against the numpy
reference (resample_ref).  Every comparison is by bytes: the filter is specified to the last float32 bit."""
import numpy as np
import pytest

from vent_analysis_amd import _lib

import mask_edit_ref as M
import register_ref as G
import resample_ref as F
import segment_ref as S

pytestmark = pytest.mark.gpu

VOX = (1.5, 1.5, 10.0)
DST = (41, 37, 9)


def same(a, b):
    """Equal dtype, shape and bits."""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def where_differs(a, b):
    return np.argwhere(np.asarray(a).view(np.uint32) != np.asarray(b).view(np.uint32))[:4].tolist()


def resampled(src, dst_shape, maps):
    """Through a batch of its own: (the resident proton after the resampling, the resident source)."""
    B = _lib.Batch(*dst_shape, len(src))
    B.upload_proton_src(src)
    used = B.resample_proton(maps)
    out, back = B.download_proton(), B.download_proton_src()
    B.close()
    assert used.dtype == np.float64 and used.shape == (len(src), 3, 2)
    return out, back


@pytest.mark.parametrize("src_shape,dst_shape", list(F.CASES), ids=lambda v: str(v).replace(" ", ""))
def test_resample_equals_the_reference(src_shape, dst_shape):
    src, maps = F.batch(src_shape, dst_shape)
    want = F.reference(src_shape, dst_shape)
    assert np.isfinite(want).all()
    got, back = resampled(src, dst_shape, maps)
    assert got.dtype == np.float32 and got.shape == (len(src),) + dst_shape
    assert same(got, want), where_differs(got, want)
    assert same(back, src)                                               # the source stays resident, untouched
    if src_shape == (64, 40, 12):                                        # part of the output outside the source
        assert (want[3, :20] == 0).all() and want[3, 30:].all() and (want[1, 0] == 0).all() and want[1, 8:, 8:, 4:].all()
    if src_shape == (83, 75, 9):
        assert same(_lib.resample(src, dst_shape, maps), want)           # the host-buffer form
        assert same(_lib.resample(src[1], dst_shape, maps[1])[0], want[1])   # one 3-D volume, one map


def test_tiles_bands_and_the_lds_budget(monkeypatch):
    """More than one column tile, slice tile and band, a last tile of each that is not full, and the
    smallest and the largest stage the kernel may be given: the same bits."""
    src_shape, dst_shape = (40, 50, 70), (37, 45, 67)
    src, maps = F.batch(src_shape, dst_shape)
    want = F.reference(src_shape, dst_shape)
    for kb in (None, "1", "64"):
        if kb is None:
            monkeypatch.delenv("VH_RS_LDS_KB", raising=False)
        else:
            monkeypatch.setenv("VH_RS_LDS_KB", kb)
        got, _ = resampled(src, dst_shape, maps)
        assert same(got, want), (kb, where_differs(got, want))


@pytest.mark.parametrize("dst_shape", [(7, 1024, 1), (7, 1030, 1), (5, 2100, 2)], ids=str)
def test_a_wide_plane_of_few_slices(dst_shape):
    """The tables of a tile take LDS per column: a single-slice plane of 1024 columns and more, at a row
    scale near 4 (8 staged rows for one destination row) and just over 2 (5), fits like any other."""
    src_shape = (28, 1024, dst_shape[2])
    src = np.stack([F.study(src_shape, 60 + q) for q in range(2)])
    cs = 1024.0 / dst_shape[1]
    maps = [[(3.9, 0.3), (cs, 0.2), (1.0, 0.0)], [(2.1, -0.4), (max(0.25, cs / 2), 3.0), (1.0, 0.0)]]
    assert int(F.taps(28, dst_shape[0], 3.9, 0.3)[1].max()) == 8
    want = F.reference_of(src, maps, dst_shape)
    assert want.all()
    got, _ = resampled(src, dst_shape, maps)
    assert same(got, want), where_differs(got, want)
    assert same(_lib.resample(src, dst_shape, maps), want)


@pytest.mark.parametrize("z_off", [-2.0, -2.25], ids=str)
@pytest.mark.parametrize("c_scale", [0.6, 1.7, 3.3], ids=str)
def test_one_and_two_z_tap_forms(c_scale, z_off):
    """Where no slice has more than one z-tap (a whole-number slice offset) or more than two (any offset at
    slice scale 1) the kernel reads a pair's taps together, in a form for at most 2, 4 or 8 c-taps: columns
    with fewer taps than the form's, with none, slices with none and slices with one tap of two."""
    src_shape, dst_shape = (30, 44, 7), (12, 11, 9)
    src = np.stack([F.study(src_shape, 20 + q) for q in range(4)])
    maps = [[(1.7, -0.4), (c_scale, off), (1.0, z_off)] for off in (0.0, 0.4, -9.5, 30.0)]   # slices 0 and 1 lie outside
    want = F.reference_of(src, maps, dst_shape)
    counts = [F.taps(44, 11, c_scale, off)[1] for off in (0.0, 0.4, -9.5, 30.0)]
    assert max(int(k.max()) for k in counts) == {0.6: 2, 1.7: 4, 3.3: 7}[c_scale] and min(int(k.min()) for k in counts) == 0
    assert F.taps(7, 9, 1.0, z_off)[1].tolist() == ([0, 0, 1, 1, 1, 1, 1, 1, 1] if z_off == -2.0 else [0, 0, 1, 2, 2, 2, 2, 2, 2])
    assert not want[:, :, :, :2].any() and want[0, :, :, 2:].all()
    got, _ = resampled(src, dst_shape, maps)
    assert same(got, want), where_differs(got, want)


def test_identity_and_integer_offsets():
    src = G.batch(DST)[0].copy()                                         # NaN, +-inf and negative voxels in study 2
    src[0, 0, 0, 0] = -0.0
    ident = [[1.0, 0.0]] * 3
    got, _ = resampled(src, DST, ident)
    assert np.array_equal(got, src, equal_nan=True) and not np.signbit(got[0, 0, 0, 0])   # -0.0 becomes +0.0
    shifts = [(0, 0, 0), (4, -4, 2), (-4, 4, -2), (-3, 0, 1)]
    maps = [[(1.0, float(d)) for d in s] for s in shifts]
    got, _ = resampled(src, DST, maps)
    want = np.stack([G.shift_image(src[q], shifts[q]) for q in range(4)])
    assert np.array_equal(got, want, equal_nan=True)
    finite = np.isfinite(want)
    assert same(np.where(finite, got, 0) + np.float32(0), np.where(finite, want, 0) + np.float32(0))


@pytest.mark.parametrize("src_shape", [(82, 74, 9), (98, 90, 11)], ids=str)
def test_a_shift_folded_into_the_map_composes_with_shift_proton(src_shape):
    """grid_map(..., shift=s) is the unshifted resampling moved by s wherever shift_proton did not pull
    zeros in; in that margin it holds the source's own data when the source's field of view covers it."""
    covers = src_shape == (98, 90, 11)
    src = np.stack([F.study(src_shape, 40 + q) for q in range(4)])
    src_vox = (0.75, 0.75, 10.0)
    base = _lib.grid_map(src_shape, src_vox, DST, VOX)
    assert base.tolist() == ([[2.0, 8.5], [2.0, 8.5], [1.0, 1.0]] if covers else [[2.0, 0.5], [2.0, 0.5], [1.0, 0.0]])
    shifts = np.array([(0, 0, 0), (3, -2, 1), (-4, 4, -1), (1, 0, 0)], np.int32)
    B = _lib.Batch(*DST, 4)
    B.upload_proton_src(src)
    B.resample_proton(base)
    plain = B.download_proton()
    B.shift_proton(shifts)
    moved = B.download_proton()
    B.resample_proton([_lib.grid_map(src_shape, src_vox, DST, VOX, shift=s) for s in shifts])   # the source is still there
    folded = B.download_proton()
    B.close()
    assert same(plain, np.stack([F.resample(src[q], DST, base) for q in range(4)]))
    inside = np.stack([G.shift_image(np.ones(DST, bool), s) for s in shifts])
    assert same(moved, np.stack([G.shift_image(plain[q], shifts[q]) for q in range(4)]))
    assert same(np.where(inside, folded, 0), np.where(inside, moved, 0))
    assert same(folded[0], plain[0]) and (~inside[1:]).any()
    if covers:
        assert (folded[~inside] != 0).all() and not moved[~inside].any()


def test_one_nan_voxel_reaches_exactly_the_outputs_whose_taps_include_it():
    src_shape = (83, 75, 9)
    src, maps = F.batch(src_shape, DST)
    clean = F.reference(src_shape, DST)
    at = (40, 31, 4)
    src = src.copy()
    src[:, at[0], at[1], at[2]] = np.nan
    got, _ = resampled(src, DST, maps)
    for q in range(4):
        hit = np.ones(DST, bool)
        for a, table in enumerate(F.tables(src_shape, DST, maps[q])):
            first, count, _ = table
            on = (first <= at[a]) & (at[a] < first + count)
            hit &= on.reshape([-1 if k == a else 1 for k in range(3)])
        assert hit.any() and not hit.all()
        assert np.array_equal(np.isnan(got[q]), hit), q
        assert same(np.where(hit, 0, got[q]), np.where(hit, 0, clean[q])), q


def fine_study(seed=0):
    """(a proton on a grid twice as fine in plane as DST, its map, the xenon on DST)."""
    src_shape = (82, 74, 9)
    return F.study(src_shape, 70 + seed), _lib.grid_map(src_shape, (0.75, 0.75, 10.0), DST, VOX), G.batch(DST)[1][0]


def test_end_to_end_resample_register_segment():
    protons = np.stack([fine_study(q)[0] for q in range(4)])
    X = G.batch(DST)[1]
    planted = [(2, -1, 0), (-2, 2, 1), (0, 1, -1), (1, 0, 0)]          # the proton lies off the xenon by these
    maps = [_lib.grid_map(protons.shape[1:], (0.75, 0.75, 10.0), DST, VOX, shift=tuple(-d for d in s)) for s in planted]
    on_grid = np.stack([F.resample(p, DST, m) for p, m in zip(protons, maps)])
    search = (2, 2, 1)
    _, _, rbest, gaps = G.reference_of(on_grid, X, search)
    assert rbest == planted and min(gaps) >= 1e-6                       # the reference first
    B = _lib.Batch(*DST, 4)
    B.upload(X, np.ones((4,) + DST, np.uint8))
    B.upload_proton_src(protons)
    B.resample_proton(maps)
    best = B.register(search)[0]
    assert [tuple(b) for b in best] == rbest
    B.shift_proton(best)
    B.segment(50.0, open_radius=1)
    got = B.download_mask()
    B.close()
    want = np.stack([S.segment(G.shift_image(on_grid[q], rbest[q]), 50.0, 1) for q in range(4)])
    assert want.any() and same(got, want)


def test_class_method_then_segment_mask():
    from vent_analysis_amd import Vent_Analysis
    proton, m, xenon = fine_study()
    va = Vent_Analysis(pickle_dict=dict(HPvent=xenon.copy(), mask=np.ones(DST), vox=list(VOX)))
    keys = set(vars(va))
    va.proton = proton.astype(np.float64)
    out = va.resample_proton(proton_vox=(0.75, 0.75, 10.0))
    want = F.resample(proton, DST, m)
    assert out is va.proton and same(va.proton, want)
    assert set(vars(va)) - keys <= {"proton"}
    mask = va.segment_mask(thresh=50.0)
    assert same(np.asarray(mask, np.uint8), S.segment(want, 50.0, 1)) and mask.any()
    assert isinstance(va.register_proton((1, 1, 0), apply=False)[0], tuple)          # it takes the proton now
    va.proton = proton
    shifted = va.resample_proton(proton_vox=(0.75, 0.75, 10.0), shift=(2, -1, 0))
    assert same(shifted, F.resample(proton, DST, _lib.grid_map(proton.shape, (0.75, 0.75, 10.0), DST, VOX, (2, -1, 0))))


def test_state_and_library_argument_errors():
    src_shape = (83, 75, 9)
    src, maps = F.batch(src_shape, DST)
    masks = M.batch_masks(DST)
    X = np.abs(np.nan_to_num(G.batch(DST)[1], nan=1.0, posinf=2.0, neginf=3.0)) + np.float32(5)
    p = _lib._ptr
    ERR = _lib.VH_ERR_ARG
    B = _lib.Batch(*DST, 4)
    B.upload(X, masks)
    B.run(B.options(do_n4=False, vox=VOX))
    before = B.download()
    mp = np.ascontiguousarray(maps)
    shape = np.asarray(src_shape, np.int64)
    assert B.L.vh_batch_resample_proton(B.h, p(mp)) == ERR                                  # no source resident
    assert B.L.vh_batch_download_proton_src(B.h, p(np.zeros_like(src))) == ERR
    with pytest.raises(ValueError):
        B.resample_proton(maps)
    with pytest.raises(ValueError):
        B.download_proton_src()
    for call in (B.register, lambda: B.segment(50.0)):
        with pytest.raises(ValueError, match="no proton resident"):
            call()
    assert B.L.vh_batch_upload_proton_src(B.h, None, p(shape)) == ERR
    assert B.L.vh_batch_upload_proton_src(B.h, p(src), None) == ERR
    for bad in ((0, 75, 9), (83, 1025, 9), (83, 75, -1)):
        assert B.L.vh_batch_upload_proton_src(B.h, p(src), p(np.asarray(bad, np.int64))) == ERR, bad
    assert B.L.vh_batch_resample_proton(B.h, p(mp)) == ERR                                  # still none
    B.upload_proton_src(src)
    assert B.L.vh_batch_resample_proton(B.h, None) == ERR
    assert B.L.vh_batch_download_proton_src(B.h, None) == ERR
    for q, a, k, v in ((0, 0, 0, 0.2), (3, 2, 0, 4.5), (1, 1, 0, np.nan), (2, 0, 1, np.inf), (3, 2, 1, -2.0 ** 20 - 1),
                       (0, 1, 1, np.nan)):
        bad = mp.copy()
        bad[q, a, k] = v
        assert B.L.vh_batch_resample_proton(B.h, p(bad)) == ERR, (q, a, k, v)
    with pytest.raises(ValueError, match="no proton resident"):                             # nothing was enqueued
        B.register()
    B.resample_proton(maps)
    want = F.reference(src_shape, DST)
    assert same(B.download_proton(), want)
    B.register((1, 1, 0))                                                                    # no longer raise
    after = B.download()                                                                     # a run's results survive
    for a, b in zip(before[:4], after[:4]):
        assert (a is None and b is None) or same(a, b)
    assert [r.n_mask for r in before[4]] == [r.n_mask for r in after[4]]
    assert same(B.download_mask(), masks) and same(B.download_hp(), X) and same(B.download_proton_src(), src)
    B.upload_proton(want[::-1].copy())                                                       # an upload replaces it,
    B.resample_proton(maps[0])                                                               # one map for every study
    assert same(B.download_proton(), F.reference_of(src, [maps[0]] * 4, DST))
    small = np.ascontiguousarray(src[:, :21, :19, :5])                                      # another source shape
    B.upload_proton_src(small)
    B.resample_proton(F.CASES[((21, 19, 5), DST)])
    assert same(B.download_proton(), F.reference_of(small, F.CASES[((21, 19, 5), DST)], DST))
    assert same(B.download_proton_src(), small)
    B.segment(50.0)
    B.close()
    c = _lib.context(0)
    out = np.zeros((4,) + DST, np.float32)
    args = (41, 37, 9, 4, p(mp), p(out))
    assert c.L.vh_resample(c.h, None, p(shape), *args) == ERR
    assert c.L.vh_resample(c.h, p(src), None, *args) == ERR
    assert c.L.vh_resample(c.h, p(src), p(shape), 41, 37, 9, 4, None, p(out)) == ERR
    assert c.L.vh_resample(c.h, p(src), p(shape), 41, 37, 9, 4, p(mp), None) == ERR
    assert c.L.vh_resample(c.h, p(src), p(np.asarray((83, 75, 2000), np.int64)), *args) == ERR
    assert not out.any()
