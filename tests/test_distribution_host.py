"""CPU: the distribution calls exist at every layer (header, library, ctypes), refuse a null batch
without touching a device, and the numpy reference the GPU tests compare against is itself pinned:
against the cohort rows, against the oracle's counts and against stored counts of one input."""
import ctypes as ct
import os
import re

import numpy as np
import pytest

from conftest import REPO
from oracle import vdp_oracle as O
from vent_analysis_amd import _lib

import distribution_ref as R
import standin_lib

NEW = ("vh_batch_distribution", "vh_batch_download_distribution", "vh_distribution")
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
    for name, val in (("VH_NORM_MEAN", 0), ("VH_NORM_P99", 1), ("VH_DIST_COLS", 8)):
        assert re.search(r"^#define %s\s+%d\b" % (name, val), hdr, re.M), name
        assert getattr(_lib, name) == val
    assert L.vh_batch_kernel_names().decode() == NAMES   # "dist_b" is timed but not listed
    assert L.vh_abi_version() == 8   # additions only


def test_null_batch_is_an_argument_error():
    """Checked before anything is dereferenced: no device is needed."""
    L = _lib.lib()
    buf = np.zeros(64, np.uint8)
    p = _lib._ptr(buf)
    assert L.vh_batch_distribution(None, 1, 1024, ct.c_float(1.5)) == _lib.VH_ERR_ARG
    assert L.vh_batch_download_distribution(None, p, p, p) == _lib.VH_ERR_ARG
    assert L.vh_distribution(None, p, p, 2, 2, 2, 1, ct.c_float(0.6), 1, 4, ct.c_float(1.5), p, p,
                             p) == _lib.VH_ERR_ARG


def test_norm_names():
    assert [_lib.norm_source(s) for s in ("mean", "p99", 0, 1, np.int64(1))] == [0, 1, 0, 1, 1]
    for bad in ("p", "P99", "lb", 0.5, None):
        with pytest.raises((ValueError, TypeError)):
            _lib.norm_source(bad)
    e = _lib.dist_edges(100, 1.5)
    assert e.dtype == np.float64 and e.shape == (101,) and e[0] == 0 and e[-1] == 100 * (1.5 / 100)


def test_ventilation_distribution_needs_calculate_vdp():
    """Called before calculate_VDP it raises, like select_defect; no device is touched and the object
    stays as it was."""
    from vent_analysis_amd import Vent_Analysis
    X, M = R.D.field((7, 5, 3), 1)
    va = Vent_Analysis(pickle_dict=dict(HPvent=X, mask=M.astype(np.float64), vox=[1.5, 1.5, 10.0]))
    assert hasattr(Vent_Analysis, "ventilation_distribution")
    before = {k: (v.copy() if isinstance(v, (np.ndarray, dict)) else v) for k, v in vars(va).items()}
    with pytest.raises(ValueError):
        va.ventilation_distribution()
    assert set(vars(va)) == set(before)
    np.testing.assert_equal({k: v for k, v in vars(va).items()}, before)
    assert isinstance(va.N4HPvent, str) and isinstance(va.defectArray, str)


# ---- the reference itself ------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(41, 37, 9), (7, 5, 3)], ids=str)
def test_p99_rows_sum_to_the_cohort(shape):
    """With (p99, 1024, 1.5) a study's row is the cohort's row of it (k_cohort_search): summed over
    the batch they are standin_lib.cohort_rows.  (cohort_rows indexes the sorted masked list, so the
    empty-mask study stays out: its row is zero.)"""
    hp, mk, _, _ = R.batch_inputs(shape)
    refs = R.batch_reference(shape, "p99", 1024, 1.5)
    keep = [q for q in range(hp.shape[0]) if mk[q].any()]
    assert len(keep) == hp.shape[0] - 1 and not refs[2]["hist"].any() and not refs[2]["outside"].any()
    with np.errstate(divide="ignore", invalid="ignore"):
        rows = standin_lib.cohort_rows(hp[keep], mk[keep])
    assert np.array_equal(sum(refs[q]["hist"].astype(np.int64) for q in keep), rows)
    assert rows.sum() > 0


@pytest.mark.parametrize("norm", R.NORMS)
@pytest.mark.parametrize("bins,hi", R.PARAMS)
@pytest.mark.parametrize("shape", R.SHAPES + [R.TALL], ids=str)
def test_reference_invariants(shape, bins, hi, norm):
    hp, mk, defect, lb = R.batch_inputs(shape)
    refs = R.batch_reference(shape, norm, bins, hi)
    for q, r in enumerate(refs):
        n_mask = int((mk[q] != 0).sum())
        sl = r["slice_counts"]
        assert r["hist"].shape == (bins,) and r["hist"].dtype == np.uint32
        assert sl.shape == (shape[2], R.COLS) and sl.dtype == r["outside"].dtype == np.int64
        assert int(r["hist"].sum()) + int(r["outside"].sum()) == n_mask, q
        assert int(sl[:, 0].sum()) == n_mask
        if q != 6:   # (every masked value 0: the classes are NaN's, 0)
            assert np.array_equal(sl[:, 2:].sum(axis=1), sl[:, 0]), q   # 0/1 masks: one class per voxel
        else:
            assert not sl[:, 2:].any() and r["outside"][1] == n_mask and not r["hist"].any()
        if n_mask and q != 6:
            o = O.calculate_vdp(hp[q], mk[q], R.VOX)
            assert int(sl[:, 2:4].sum()) == int(np.isin(o["defectArrayLB"], (1, 2)).sum()), q   # n_lb12
            assert int(sl[:, 1].sum()) == int(o["defectArray"].sum()), q
    assert refs[5]["outside"][0] > 0   # the negated values
    assert not refs[2]["slice_counts"].any()   # the empty mask


def test_field_counts():
    """Input drift is noticed: counts of the seed-1 field at (41, 37, 9)."""
    r = R.batch_reference((41, 37, 9), "p99", 100, 1.5)[0]
    m = R.batch_reference((41, 37, 9), "mean", 7, 2.0)[0]
    sl = r["slice_counts"]
    got = (int(sl[:, 0].sum()), int(sl[:, 1].sum()), tuple(int(x) for x in sl[:, 2:].sum(axis=0)),
           tuple(int(x) for x in r["outside"]), int(r["hist"][:10].sum()), int(r["hist"].argmax()),
           tuple(int(x) for x in m["hist"]), tuple(int(x) for x in m["outside"]),
           tuple(int(x) for x in sl[4]))
    assert got == FIELD_COUNTS, got


# n_mask, defect voxels, the six LB classes, outside, hist[:10].sum(), hist.argmax() of (p99, 100,
# 1.5); hist and outside of (mean, 7, 2.0); slice 4's row
FIELD_COUNTS = (9873, 534, (30, 659, 2842, 3930, 1956, 456), (0, 0), 25, 37,
                (40, 604, 2519, 3739, 2216, 665, 85), (0, 5), (1097, 90, 0, 101, 338, 410, 212, 36))
