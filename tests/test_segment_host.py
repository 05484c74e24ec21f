"""CPU: the proton-segmentation calls exist at every layer (header, library, ctypes, class) and refuse
bad arguments without touching a device; vh_otsu, a host function, equals the exact-rational cut; the
numpy reference the GPU tests compare against (segment_ref) is scipy.ndimage's binary_fill_holes and
binary_opening; and the shared inputs are such that no step is trivial on them."""
import ctypes as ct
import os
import re

import numpy as np
import pytest

from conftest import REPO
from vent_analysis_amd import _lib

import mask_edit_ref as M
import segment_ref as S

NEW = ("vh_batch_upload_proton", "vh_batch_proton_threshold", "vh_batch_segment", "vh_batch_mask_overlap",
       "vh_otsu", "vh_segment")
NAMES = ("mask_stats;gather;sort;mean;classify;cohort;kmeans;snr;border;n4_init;n4_den;n4_hist;"
         "n4_fit;n4_contract;n4_eval;n4_welford;n4_pcw;n4_pcg;n4_final;n4_study;ci_walk;vdp_chain;"
         "ci_walk_b;defect_sel")
ALL_SHAPES = S.SHAPES + [S.BIG]


def studies(shape):
    return 2 if shape == S.BIG else 4


def test_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(REPO, "include", "vent_hip.h")).read()
    L = _lib.lib()
    for n in NEW:
        assert re.search(r"^int %s\((vh_(batch|ctx) \*|const uint32_t \*hist)" % n, hdr, re.M), n
        assert hasattr(L, n), n
        assert n in _lib._SIGS, n
    assert "Vent_Analysis.py:1024" in hdr and "binary_fill_holes" in hdr
    assert L.vh_batch_kernel_names().decode() == NAMES   # "segment_b" is timed but not listed
    assert L.vh_abi_version() == 8   # additions only
    for n in ("upload_proton", "proton_threshold", "segment", "mask_overlap"):
        assert callable(getattr(_lib.Batch, n)), n
    assert callable(_lib.segment) and callable(_lib.otsu) and callable(_lib._segment_args)
    from vent_analysis_amd import Vent_Analysis
    assert callable(Vent_Analysis.segment_mask)
    doc = " ".join(Vent_Analysis.segment_mask.__doc__.split())
    assert "calculate_VDP" in doc and "old mask" in doc


def test_null_handles_are_argument_errors():
    """Checked before anything is dereferenced: no device is needed."""
    L = _lib.lib()
    f32, u8 = np.ones(64, np.float32), np.ones(64, np.uint8)
    rad, cnt, h = np.ones(4, np.int32), np.zeros(12, np.int64), np.zeros(4 * 256, np.uint32)
    p = _lib._ptr
    assert L.vh_batch_upload_proton(None, p(f32)) == _lib.VH_ERR_ARG
    assert L.vh_batch_proton_threshold(None, p(f32), p(f32), p(h)) == _lib.VH_ERR_ARG
    assert L.vh_batch_segment(None, p(f32), p(rad)) == _lib.VH_ERR_ARG
    assert L.vh_batch_mask_overlap(None, p(u8), p(cnt)) == _lib.VH_ERR_ARG
    assert L.vh_segment(None, p(f32), 2, 2, 2, 1, p(f32), p(rad), p(u8), p(f32), p(cnt)) == _lib.VH_ERR_ARG
    k = ct.c_int32(7)
    assert L.vh_otsu(None, 256, ct.byref(k)) == _lib.VH_ERR_ARG
    assert L.vh_otsu(p(h), 256, None) == _lib.VH_ERR_ARG
    assert L.vh_otsu(p(h), 1, ct.byref(k)) == _lib.VH_ERR_ARG and k.value == 7


@pytest.mark.parametrize("thresh,radius,n,shape", [
    (1.0, -1, 2, None), (1.0, 6, 2, None), (1.0, 2.5, 2, None), (1.0, [1, 2, 3], 2, None), (1.0, [1, 6], 2, None),
    (1.0, True, 2, None), (1.0, [[1, 2]], 2, None), (np.nan, 1, 2, None), (0.0, 1, 2, None), (-3.0, 1, 2, None),
    (np.inf, 1, 2, None), ([1.0, np.nan], 1, 2, None), ([1.0, 2.0, 3.0], 1, 2, None), ("a", 1, 2, None),
    (True, 1, 2, None), (1.0, 1, 2, (8, 513, 4)), (1.0, 1, 2, (513, 8, 4)), (None, 6, 2, None)], ids=str)
def test_argument_errors_are_value_errors(thresh, radius, n, shape):
    """The checks of vh_batch_segment, made by the binding first: ValueError, no device call."""
    with pytest.raises(ValueError):
        _lib._segment_args(thresh, radius, n, shape)


def test_argument_forms():
    th, rad = _lib._segment_args(None, 1, 3)
    assert th is None and rad.dtype == np.int32 and rad.tolist() == [1, 1, 1]
    th, rad = _lib._segment_args(2, (0, 5, 2), 3, (512, 512, 1))
    assert th.dtype == np.float32 and th.flags.c_contiguous and th.tolist() == [2.0, 2.0, 2.0]
    assert rad.flags.c_contiguous and rad.tolist() == [0, 5, 2]
    th, _ = _lib._segment_args(np.array([0.5, 40.0]), np.int64(0), 2)
    assert th.tolist() == [0.5, 40.0]


# ---- vh_otsu ---------------------------------------------------------------------------------------
def lib_otsu(h):
    h = np.ascontiguousarray(h, np.uint32)
    k = ct.c_int32(-7)
    rc = _lib.lib().vh_otsu(_lib._ptr(h), h.size, ct.byref(k))
    return rc, k.value


def test_otsu_hand_cases():
    h = np.zeros(256, np.uint32)
    h[10], h[200] = 5, 9                  # two occupied bins: every cut between them ties -> the lowest
    assert lib_otsu(h) == (_lib.VH_OK, 10) and S.otsu_exact(h) == 10 and _lib.otsu(h) == 10
    h[:] = 0
    h[3:6], h[100:103] = (4, 9, 4), (4, 9, 4)     # empty bins between two modes: ties -> the lowest k
    assert lib_otsu(h) == (_lib.VH_OK, 5) and S.otsu_exact(h) == 5
    h[:] = 0
    h[0], h[255] = 1, 1
    assert lib_otsu(h) == (_lib.VH_OK, 0)
    h[:] = 0
    h[254], h[255] = 3, 1                 # the last possible cut
    assert lib_otsu(h) == (_lib.VH_OK, 254)
    h[:] = 0
    h[77] = 1000                          # one occupied bin
    assert lib_otsu(h) == (_lib.VH_ERR_EMPTY, -7) and S.otsu_exact(h) is None and S.otsu_double(h) is None
    with pytest.raises(IndexError):
        _lib.otsu(h)
    assert lib_otsu(np.zeros(256, np.uint32))[0] == _lib.VH_ERR_EMPTY
    assert lib_otsu(np.array([2, 0, 1, 7], np.uint32)) == (_lib.VH_OK, S.otsu_exact([2, 0, 1, 7]))
    assert lib_otsu(np.array([0xffffffff, 0xffffffff, 1], np.uint32))[0] == _lib.VH_OK    # no 32-bit overflow
    with pytest.raises(ValueError):
        _lib.otsu(np.zeros((2, 4)))


def test_otsu_equals_the_exact_cut_on_every_test_histogram():
    """The library's double arg-max, the reference's double arg-max and the exact-rational arg-max agree
    on the histogram of every study of every shape; and they can: the best and the second-best distinct
    values of the criterion differ by more than 1e-9 relative, a million times the rounding of the three
    double operations behind a value (the sums are exact integers below 2^53 at these sizes)."""
    rng = np.random.default_rng(5)
    hists = [(shape, q, S.batch_stats(shape, studies(shape))[2][q]) for shape in ALL_SHAPES
             for q in range(studies(shape))]
    hists += [("random", i, rng.integers(0, 5000, 256).astype(np.uint32)) for i in range(4)]
    for shape, q, h in hists:
        exact = S.otsu_exact(h)
        assert exact is not None, (shape, q)
        assert lib_otsu(h) == (_lib.VH_OK, exact), (shape, q)
        assert S.otsu_double(h) == exact, (shape, q)
        margin = S.otsu_margin(h)
        assert margin is None or margin > 1e-9, (shape, q, margin)
        assert int(np.sum(h.astype(np.int64) * np.arange(256))) * int(h.sum()) < 2 ** 53


# ---- the reference itself --------------------------------------------------------------------------
def test_statistics_of_special_values():
    x = np.array([np.nan, np.inf, -np.inf, -1.0, -0.0, 0.0, 1.0, 2.0, 4.0], np.float32)
    pmax, hist = S.stats(x)
    assert pmax == 4.0 and hist.sum() == 5            # -0.0, 0.0, 1.0, 2.0, 4.0
    assert hist[0] == 2 and hist[64] == 1 and hist[128] == 1 and hist[255] == 1
    for empty in (np.zeros(5, np.float32), np.array([np.nan, -2.0, np.inf], np.float32)):
        pmax, hist = S.stats(empty)
        assert pmax == 0 and not hist.any() and np.isnan(S.threshold(empty))
    assert np.isnan(S.threshold(np.full(9, 3.0, np.float32)))     # one occupied bin
    t = S.threshold(x)
    assert t.dtype == np.float32 and t == np.float32(S.otsu_exact(S.stats(x)[1]) + 1) * np.float32(4.0 / 256.0)


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=str)
def test_the_reference_is_scipys_fill_holes_and_opening(shape):
    ndi = pytest.importorskip("scipy.ndimage")
    n = studies(shape)
    x = S.batch_proton(shape)[:n]
    for otsu in (False, True):
        ts = S.batch_stats(shape, n)[0] if otsu else S.THRESH[:n]
        seg = S.batch_unopened(shape, otsu, n)
        for q in range(n):
            with np.errstate(invalid="ignore"):
                dark = x[q] < np.float32(ts[q])
            want = np.stack([ndi.binary_fill_holes(~dark[:, :, z]) & dark[:, :, z] for z in range(shape[2])], axis=2)
            assert np.array_equal(seg[q] != 0, want), (otsu, q)
    seg = S.batch_unopened(shape, False, n)
    for k in (1, 2, 5):
        d = np.zeros((2 * k + 1, 2 * k + 1), bool)
        for dr, dc in M.disc(k):
            d[k + dr, k + dc] = True
        for q in range(n):
            got = S.batch_reference(shape, (k,) * n, False, n)[q]
            ero = ndi.binary_erosion(seg[q] != 0, structure=d[:, :, None], border_value=1)
            assert np.array_equal(got != 0, ndi.binary_dilation(ero, structure=d[:, :, None])), (k, q)
            if not (ero[0].any() or ero[-1].any() or ero[:, 0].any() or ero[:, -1].any()):
                want = np.stack([ndi.binary_opening(seg[q][:, :, z] != 0, structure=d) for z in range(shape[2])], axis=2)
                assert np.array_equal(got != 0, want), (k, q)    # (scipy's opening erodes with pad 0)


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=str)
def test_the_inputs_are_as_described(shape):
    n = studies(shape)
    R, C, Z = shape
    x = S.batch_proton(shape)
    assert x.dtype == np.float32 and x.shape == (4,) + shape and not x.flags.writeable
    assert x is S.batch_proton(shape)
    th = S.batch_stats(shape, n)[0]
    assert np.isfinite(th).all() and (th > 0).all()
    assert 20 < th[0] < 80                                   # Otsu lands between the lungs and the body
    # study 0: neither empty nor full, the opening removes something, the slices differ
    for otsu in (False, True):
        s0 = S.batch_unopened(shape, otsu, n)[0]
        assert s0.any() and not s0.all()
        o1 = S.batch_reference(shape, (1,) * n, otsu, n)[0]
        assert o1.any() and not np.array_equal(o1, s0)
        assert any(not np.array_equal(s0[:, :, z], s0[:, :, 0]) for z in range(1, Z))
    # study 1: the maze
    L, Sd = (R, C) if R >= C else (C, R)
    dark, runs, wall, corr, (r0, c0) = S.maze_layout(L, Sd)
    assert runs - 1 >= 10                                    # U-turns
    m = x[1] if R >= C else x[1].transpose(1, 0, 2)
    assert np.isnan(m[wall]).all() and (m[corr] == -np.inf).all() and (m[5, Sd // 2] == np.inf).all()
    assert set(np.unique(m[np.isfinite(m)])) == {0.0, 1.0}
    seg = S.batch_unopened(shape, False, n)[1]
    seg = seg if R >= C else seg.transpose(1, 0, 2)
    corridor = dark.copy()
    corridor[L - 10:] = False
    diamond = np.zeros_like(dark)
    for dr in range(-2, 3):
        w = 2 - abs(dr)
        diamond[r0 + dr, c0 - w:c0 + w + 1] = True
    for z in range(Z):
        want = diamond | corridor if z % 2 else diamond       # the wall holds; the open corridor floods
        assert np.array_equal(seg[:, :, z] != 0, want), z
        assert not seg[wall + (z,)] and not seg[5, Sd // 2, z]  # NaN and +inf are not dark
    assert seg[corr + (1,)] == 1                                 # -inf is
    with np.errstate(invalid="ignore"):
        rounds = S.flood(m[:, :, 0] < 0.5)[1]
    assert rounds > 8, rounds
    # study 2 is all dark, study 3 is its interior but for the slice whose frame is open
    if n == 4:
        s = S.batch_unopened(shape, False, n)
        assert not s[2].any()
        z1 = min(1, Z - 1)
        for z in range(Z):
            if z == z1:
                assert not s[3][:, :, z].any()
            else:
                assert s[3][1:-1, 1:-1, z].all() and s[3][:, :, z].sum() == (R - 2) * (C - 2)


def test_flood_hand_cases():
    d = np.zeros((5, 6), bool)
    d[1:4, 1:5] = True                   # enclosed
    assert not S.flood(d)[0].any() and S.flood(d)[1] == 0
    d[0, 2] = True                       # opened
    assert np.array_equal(S.flood(d)[0], d)
    d[:] = True
    d[1, 2] = d[2, 1] = d[2, 3] = d[3, 2] = False      # a diagonal wall round (2, 2)
    r = S.flood(d)[0]
    assert not r[2, 2] and r.sum() == d.sum() - 1
    assert S.segment(np.where(d, 0, 1).astype(np.float32)[:, :, None], 0.5)[2, 2, 0] == 1


def test_the_packing_widths_that_fit():
    assert [z for z in S.ZCS if S.zc_fits(S.BIG, z)] == [1, 2]
    for shape in S.SHAPES:
        assert all(S.zc_fits(shape, z) for z in S.ZCS)
    assert S.zc_fits((128, 128, 24), 32) and not S.zc_fits((256, 256, 24), 32)
