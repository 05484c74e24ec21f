"""CPU: the core-rind calls exist at every layer (header, library, ctypes, class) and refuse bad
arguments without touching a device; the numpy reference the GPU tests compare against (core_rind_ref)
is scipy.ndimage's exact Euclidean distance transform of the 0-padded slice, squared, and agrees with
the erosion of mask_edit_ref; and the shared inputs reach every band."""
import ctypes as ct
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO
from vent_analysis_amd import _lib

import core_rind_ref as K
import mask_edit_ref as ME

NEW = ("vh_batch_core_rind", "vh_batch_download_core_rind", "vh_core_rind")
NAMES = ("mask_stats;gather;sort;mean;classify;cohort;kmeans;snr;border;n4_init;n4_den;n4_hist;"
         "n4_fit;n4_contract;n4_eval;n4_welford;n4_pcw;n4_pcg;n4_final;n4_study;ci_walk;vdp_chain;"
         "ci_walk_b;defect_sel")
SMALL = [s for s in K.SHAPES if s != (300, 280, 2) and s != (33, 40, 33)]   # every shape up to (130, 19, 2)


def test_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(REPO, "include", "vent_hip.h")).read()
    L = _lib.lib()
    for n in NEW:
        assert re.search(r"^int %s\(vh_(batch|ctx) \*" % n, hdr, re.M), n
        assert hasattr(L, n), n
        assert n in _lib._SIGS, n
    assert re.search(r"^int vh_core_rind_form\(int64_t R, int64_t C, int64_t Z\);", hdr, re.M)
    assert "unlike the erosion" in hdr and "pads with 1" in hdr     # the header says how the border differs
    assert L.vh_batch_kernel_names().decode() == NAMES              # "depth_b" is timed but not listed
    assert L.vh_abi_version() == 8                                  # additions only
    for n in ("core_rind", "download_core_rind"):
        assert callable(getattr(_lib.Batch, n)), n
    assert callable(_lib.core_rind) and callable(_lib.depth_thresholds) and callable(_lib.band_vdp)
    from vent_analysis_amd import Vent_Analysis
    assert callable(Vent_Analysis.core_rind)
    assert "sets nothing on the object" in Vent_Analysis.core_rind.__doc__


def test_null_arguments_are_argument_errors():
    """Checked before anything is dereferenced: no device is needed."""
    L = _lib.lib()
    buf = np.ones(64, np.uint16)
    p = _lib._ptr(buf)
    assert L.vh_batch_core_rind(None, p, 1, 0) == _lib.VH_ERR_ARG
    assert L.vh_batch_download_core_rind(None, p, p, p) == _lib.VH_ERR_ARG
    assert L.vh_core_rind(None, p, None, 2, 2, 2, 1, p, 1, p, p, p) == _lib.VH_ERR_ARG


def test_the_form_predicate():
    """Host only.  The search runs on rows staged in LDS while a row of C Z column distances -- bytes
    where R <= 510, uint16 above -- fits 60 KiB; a longer row takes the form that reads them through
    the caches."""
    import core_rind_ref
    for shape in core_rind_ref.SHAPES + [(128, 128, 24), (520, 516, 1)]:
        assert _lib.core_rind_form(*shape) == "rows", shape
    assert _lib.core_rind_form(*core_rind_ref.LONG_ROW) == "global"
    assert _lib.core_rind_form(510, 61440, 1) == "rows" and _lib.core_rind_form(510, 61441, 1) == "global"
    assert _lib.core_rind_form(511, 30720, 1) == "rows" and _lib.core_rind_form(511, 30721, 1) == "global"
    assert _lib.core_rind_form(3, 2048, 30) == "rows" and _lib.core_rind_form(3, 2049, 30) == "global"
    with pytest.raises(ValueError):
        _lib.core_rind_form(0, 4, 4)


def test_depth_thresholds():
    t = _lib.depth_thresholds((1.5, 3.5, 8))
    assert t.dtype == np.uint16 and t.tolist() == [3, 13, 64]
    assert _lib.depth_thresholds(()).shape == (0,) and _lib.depth_thresholds([]).dtype == np.uint16
    assert _lib.depth_thresholds(2).tolist() == [4]                       # a scalar is one edge
    assert _lib.depth_thresholds((1, 1.0001, 2 ** 0.5, 255.99)).tolist() == [1, 2, 3, 65531]
    assert _lib.depth_thresholds((0.1, 1.2)).tolist() == [1, 2]           # D2 >= 0.01 is D2 >= 1
    assert _lib.depth_thresholds((255.998,)).tolist() == [65535]
    assert _lib.depth_thresholds(np.sqrt(np.arange(1, 32)) - 1e-9).tolist() == list(range(1, 32))   # 31 edges
    # D2 >= e^2  <=>  D2 >= ceil(e^2), for every integer D2 around it
    for e in (1.5, 2.0, 3.3, 7.75):
        thr = int(_lib.depth_thresholds((e,))[0])
        d2 = np.arange(0, 80)
        assert np.array_equal(d2 >= e * e, d2 >= thr)


@pytest.mark.parametrize("edges", [(0.0,), (-1.0,), (np.nan,), (np.inf,), (1.0, np.inf), (256.0,), (1e6,),
                                   (2.0, 2.0), (3.0, 2.0), (1.1, 1.2), tuple(range(1, 33)), ((1.0, 2.0),)],
                         ids=str)
def test_depth_threshold_errors(edges):
    """Not finite, not positive, a threshold above 65535, duplicate (or decreasing) thresholds -- 1.1
    and 1.2 both give 2 --, more than 31 edges, not a flat sequence."""
    with pytest.raises(ValueError):
        _lib.depth_thresholds(edges)


def test_argument_helper():
    h = _lib._core_rind_args
    assert h((1.5, 3.5), None).tolist() == [3, 13]
    assert h((1.5, 3.5), (2,)).tolist() == [2] and h((1.5,), ()).shape == (0,)     # thresholds win
    t = h(None, np.arange(1, 32))
    assert t.dtype == np.uint16 and t.tolist() == list(range(1, 32))
    assert h(None, [1, 65535]).tolist() == [1, 65535]
    for bad in ((0,), (0, 1), (2, 2), (3, 2), (1, 65536), (-1,), tuple(range(1, 33)), (1.0, 2.0), (True,),
                ((1, 2),)):
        with pytest.raises(ValueError):
            h(None, bad)
    with pytest.raises(ValueError):
        h((0.0,), None)


def test_band_vdp():
    c = np.array([[[4, 1], [0, 0], [8, 8]], [[0, 0], [3, 0], [1, 1]]], np.int64)
    v = _lib.band_vdp(c)
    assert v.dtype == np.float64 and v.shape == (2, 3)
    assert v[0, 0] == 25.0 and np.isnan(v[0, 1]) and v[0, 2] == 100.0 and np.isnan(v[1, 0]) and v[1, 1] == 0.0


def test_class_core_rind_refusals():
    from vent_analysis_amd import Vent_Analysis
    shape = (12, 9, 1)
    mk = K.batch_masks(shape)[0].astype(np.float64)
    va = Vent_Analysis.__new__(Vent_Analysis)                # (the constructor computes the mask's border on the GPU)
    va.device, va.mask, va.defectArray, va.vox = 0, mk, '', [1.5, 1.25, 10.0]
    with pytest.raises(ValueError, match="square"):
        va.core_rind(with_defect=False)                      # anisotropic pixels
    va.vox = [1.5, 1.5, 10.0]
    with pytest.raises(ValueError, match="not set"):
        va.core_rind()                                       # no defectArray yet
    va.mask = ''
    with pytest.raises(ValueError, match="not set"):
        va.core_rind(with_defect=False)                      # no mask
    va.mask = mk
    with pytest.raises(ValueError):
        va.core_rind(edges_mm=(6.0, 3.0), with_defect=False)   # the binding's check, before any device


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_batch_state_row_under_sanitizers(tmp_path):
    """tests/core_rind_state_check.cpp, a stand-alone program over the header the library includes:
    the guard, the transition (nothing else changes), what keeps the result and what discards it."""
    csrc = os.path.join(REPO, "vent_analysis_amd", "csrc")
    exe = str(tmp_path / "chk")
    subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", csrc, os.path.join(REPO, "tests", "core_rind_state_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "core rind state ok" in r.stdout, r.stdout + r.stderr


# ---- the reference itself ------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SMALL, ids=str)
def test_the_reference_is_scipys_exact_edt_squared(shape):
    """D2 = rint(distance_transform_edt(pad(M, 1))[1:-1, 1:-1] ^ 2) on every slice of every study; and
    the reference's restriction to the clear pixels next to the mask changes nothing."""
    ndi = pytest.importorskip("scipy.ndimage")
    masks = K.batch_masks(shape) != 0
    d2 = K.batch_d2(shape)
    assert d2.dtype == np.int64
    for q in range(K.N_STUDIES):
        for z in range(shape[2]):
            M = masks[q, :, :, z]
            edt = ndi.distance_transform_edt(np.pad(M, 1))[1:-1, 1:-1]
            assert np.array_equal(d2[q, :, :, z], np.rint(edt * edt).astype(np.int64)), (q, z)
        assert np.array_equal(d2[q][~masks[q]], np.zeros((~masks[q]).sum(), np.int64))
        assert (d2[q][masks[q]] >= 1).all() and d2[q].max() <= (min(shape[:2]) // 2 + 1) ** 2
    if np.prod(shape) <= 41 * 37 * 9:
        for q in range(K.N_STUDIES):
            assert np.array_equal(K.d2_volume(masks[q], edge_only=False), d2[q]), q


def test_the_reference_on_37_by_41():
    ndi = pytest.importorskip("scipy.ndimage")
    M = ME.batch_masks((37, 41, 1))[0, :, :, 0] != 0
    edt = ndi.distance_transform_edt(np.pad(M, 1))[1:-1, 1:-1]
    assert np.array_equal(K.d2_slice(M), np.rint(edt * edt).astype(np.int64))
    assert np.array_equal(K.d2_slice(M, edge_only=False), K.d2_slice(M))


@pytest.mark.parametrize("shape", [(41, 37, 9), (64, 64, 24), (130, 19, 2)], ids=str)
def test_depth_above_k_is_the_erosion(shape):
    """{D2 > k^2} = erode(M, k), k = 1..5, on masks kept k + 1 pixels off the slice border (there the
    erosion's pad of 1 and the distance's clear ring cannot differ)."""
    for k in range(1, 6):
        m = K.border_free(K.batch_masks(shape), k)
        if k < 4 or shape != (130, 19, 2):
            assert m[0].any() and m[3].any(), (shape, k)
        for q in range(K.N_STUDIES):
            assert np.array_equal(K.d2_volume(m[q]) > k * k, ME.erode(m[q], k)), (shape, k, q)


def test_known_answers():
    """The full slice: the depth is the distance to the ring.  One clear corner pixel: the distances
    around it.  A single set pixel: 1."""
    R, C = 9, 12
    full = K.d2_slice(np.ones((R, C), bool))
    rr, cc = np.mgrid[0:R, 0:C]
    assert np.array_equal(full, np.minimum(np.minimum(rr + 1, R - rr), np.minimum(cc + 1, C - cc)) ** 2)
    assert full.max() == 25 == (min(R, C) // 2 + 1) ** 2
    M = np.ones((R, C), bool)
    M[R - 1, 0] = False
    got = K.d2_slice(M)
    assert np.array_equal(got, np.where(M, np.minimum(full, (rr - (R - 1)) ** 2 + cc ** 2), 0))
    assert got[R - 2, 1] == 2 and got[R - 3, 2] == 8 and got[4, 4] == 25      # the pixel wins, then the ring
    lone = np.zeros((R, C), bool)
    lone[4, 5] = True
    assert K.d2_slice(lone).sum() == 1


@pytest.mark.parametrize("shape", K.SHAPES[1:-1], ids=str)
def test_summary_adds_up_and_the_inputs_reach_every_band(shape):
    mk, df = K.batch_masks(shape) != 0, K.batch_defects(shape) != 0
    off = (df & ~mk).sum(axis=(1, 2, 3))                             # defect voxels off the mask
    assert (off[[0, 1, 2]] >= 4).all() and off[3] == 0 and off[4] == 1
    for thr in K.THRESHOLDS:
        maps, counts, stats = K.batch_reference(shape, thr)
        assert maps.dtype == np.uint16 and counts.shape == (K.N_STUDIES, len(thr) + 1, 2) and counts.dtype == np.int64
        for q in range(K.N_STUDIES):
            assert counts[q, :, 0].sum() == stats[q, 0] == mk[q].sum()
            assert counts[q, :, 1].sum() == (df[q] & mk[q]).sum() == df[q].sum() - off[q]
            assert stats[q, 1] == maps[q].max()                      # nothing saturates at these shapes
        assert not counts[2].any() and not stats[2].any() and not maps[2].any()   # the empty mask
        assert not K.batch_reference(shape, thr, False)[1][:, :, 1].any()
        if thr and thr[0] == 1:
            assert not counts[:, 0].any()                            # t[0] = 1: band 0 is always empty
        if thr == (3, 13, 64) and min(shape[:2]) >= 33:
            assert (counts[[0, 1, 3, 4], :3, 0] > 0).all() and (counts[[3, 4], 3, 0] > 0).all()
    rind = K.batch_reference(shape, (2,))
    assert np.array_equal(rind[1][:, 0, 0], [(m == 1).sum() for m in rind[0]])
