"""CPU: the defect-selection calls exist at every layer (header, library, ctypes), refuse a null
batch without touching a device, and the semantics the GPU tests rely on hold on the reference: the
k-means label is a function of the value, and the test field gives three different maps."""
import ctypes as ct
import os
import re

import numpy as np
import pytest

from conftest import REPO
from oracle import vdp_oracle as O
from vent_analysis_amd import _lib

import defect_select_ref as D

NEW = ("vh_batch_select_defect", "vh_batch_download_defect", "vh_batch_km_cuts", "vh_defect_map")


def test_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(REPO, "include", "vent_hip.h")).read()
    L = _lib.lib()
    for n in NEW:
        assert re.search(r"^int %s\(vh_(batch|ctx) \*" % n, hdr, re.M), n
        assert hasattr(L, n), n
        assert n in _lib._SIGS, n
    for name, val in (("VH_DEFECT_MEAN", 0), ("VH_DEFECT_LB", 1), ("VH_DEFECT_KM", 2)):
        assert re.search(r"^#define %s\s+%d$" % (name, val), hdr, re.M), name
        assert getattr(_lib, name) == val
    names = L.vh_batch_kernel_names().decode().split(";")
    assert names[-1] == "defect_sel" and names.index("ci_walk_b") == len(names) - 2   # appended
    assert L.vh_abi_version() == 8   # additions only


def test_null_batch_is_an_argument_error():
    """Checked before anything is dereferenced: no device is needed."""
    L = _lib.lib()
    buf = np.zeros(64, np.uint8)
    p = _lib._ptr(buf)
    assert L.vh_batch_select_defect(None, 0, 1) == _lib.VH_ERR_ARG
    assert L.vh_batch_download_defect(None, p, p, None, p) == _lib.VH_ERR_ARG
    assert L.vh_batch_km_cuts(None, p) == _lib.VH_ERR_ARG
    assert L.vh_defect_map(None, p, p, 2, 2, 2, 1, ct.c_float(0.6), 0, 1, p, p, None, p) == _lib.VH_ERR_ARG


def test_source_names():
    assert [_lib.defect_source(s) for s in ("mean", "lb", "kmeans", 0, 1, 2, np.int64(2))] == [0, 1, 2, 0, 1, 2, 2]
    for bad in ("km", "LB", 1.5, None):
        with pytest.raises((ValueError, TypeError)):
            _lib.defect_source(bad)


@pytest.mark.parametrize("shape", D.SHAPES, ids=str)
def test_label_is_a_function_of_the_value(shape):
    """The cuts of kmeans_1d_sorted fall between runs of equal values, so the value rule (what the
    kernels evaluate) equals the index rule (the partition itself), on every study of the batches."""
    hp, mk, refs = D.batch_reference(shape)
    for q in range(hp.shape[0]):
        on = mk[q] != 0
        if not on.any():
            assert not refs[q]["km"].any() and np.all(np.isinf(refs[q]["cuts"]))
            continue
        sig = np.sort(hp[q][on], kind="stable")
        cuts, counts = D.kmeans_cuts(sig)
        assert np.array_equal(refs[q]["km"], D.labels_by_index(hp[q], mk[q], cuts)), q
        for j in range(4):   # the labels' counts are the partition's
            assert int((refs[q]["km"] == j + 1).sum()) == int(counts[j]), (q, j)
        assert int(refs[q]["raw"]["kmeans"].sum()) == O.kmeans_low_count(counts)


def test_degenerate_partitions():
    """A constant study is one cluster; two distinct values end in clusters 0 and 3 (labels 1 and 4:
    an empty cluster's index is skipped)."""
    hp, mk, refs = D.batch_reference((41, 37, 9))
    n = int(mk[3].sum())
    assert list(refs[3]["counts"]) == [n, 0, 0, 0] and np.all(np.isinf(refs[3]["cuts"]))
    assert np.array_equal(refs[3]["km"], mk[3])
    n1, n2 = int((hp[4] == 1).sum()), int((hp[4] == 2).sum())
    assert n1 > 0 and n2 > 0 and list(refs[4]["counts"]) == [n1, 0, 0, n2]
    assert np.array_equal(refs[4]["km"], np.where(hp[4] == 2, 4, 1))
    assert list(refs[4]["cuts"]) == [2.0, 2.0, 2.0]


@pytest.mark.parametrize("shape,raw,med", [((41, 37, 9), (782, 689, 1792), (534, 463, 1407)),
                                           ((7, 5, 3), (38, 52, 25), (33, 44, 15))], ids=str)
def test_field_counts(shape, raw, med):
    """Input drift is noticed: the seed-1 field's counts (mean / lb / kmeans), raw and after the
    per-slice median; the mean-anchored median map is calculate_vdp's."""
    hp, mk, refs = D.batch_reference(shape)
    r = refs[0]
    assert tuple(int(r["raw"][s].sum()) for s in D.SOURCES) == raw
    assert tuple(int(D.filtered(r["raw"][s], 1)[0].sum()) for s in D.SOURCES) == med
    assert (r["n_lb12"], r["n_km0"]) == (raw[1], raw[2])
    o = O.calculate_vdp(hp[0], mk[0], D.VOX)
    d, bo = D.filtered(r["raw"]["mean"], 1)
    assert np.array_equal(d, o["defectArray"]) and np.array_equal(bo, o["defectBorder"])
    assert np.array_equal(r["raw"]["lb"], np.isin(o["defectArrayLB"], (1, 2)))


@pytest.mark.parametrize("shape", D.SHAPES, ids=str)
def test_three_different_nonempty_maps(shape):
    r = D.batch_reference(shape)[2][0]
    for mf in (0, 1):
        maps = [D.filtered(r["raw"][s], mf)[0] for s in D.SOURCES]
        assert all(m.any() for m in maps)
        assert not any(np.array_equal(maps[a], maps[b]) for a, b in ((0, 1), (0, 2), (1, 2)))


def test_select_defect_needs_n4hpvent():
    """Called before calculate_VDP (no N4HPvent) it raises, like the class's other methods called
    out of order; no device is touched."""
    from vent_analysis_amd import Vent_Analysis
    X, M = D.field((7, 5, 3), 1)
    va = Vent_Analysis(pickle_dict=dict(HPvent=X, mask=M.astype(np.float64), vox=[1.5, 1.5, 10.0]))
    assert hasattr(Vent_Analysis, "select_defect")
    with pytest.raises(ValueError):
        va.select_defect("kmeans")
    assert isinstance(va.defectArray, str)   # untouched
