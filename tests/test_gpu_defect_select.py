"""GPU: the defect map, border, count and k-means labels of each of calculate_VDP's three
thresholdings (vh_batch_select_defect / Batch.select_defect and the layers above it) against the CPU
reference built from oracle.vdp_oracle (defect_select_ref).  Every comparison is exact: uint8 maps,
integer counts, and cut values that are input values."""
import copy
import functools

import numpy as np
import pytest

from oracle import native, vdp_oracle as O
from vent_analysis_amd import _lib
from vent_analysis_amd.sphere import compact_table_for

import defect_select_ref as D

pytestmark = pytest.mark.gpu

VOX = D.VOX


@functools.lru_cache(maxsize=None)
def resident(shape):
    """The batch of a shape after one plain run (do_n4 = 0), kept resident for the selections of the
    parametrised cases, and that run's download."""
    hp, mk, _ = D.batch_reference(shape)
    B = _lib.Batch(*shape, hp.shape[0])
    B.upload(hp, mk)
    B.run(B.options(do_n4=False, vox=VOX))
    return B, B.download()


@pytest.mark.parametrize("medfilt", [0, 1, 2])
@pytest.mark.parametrize("source", D.SOURCES)
@pytest.mark.parametrize("shape", D.SHAPES, ids=str)
def test_selection_equals_the_reference(shape, source, medfilt):
    hp, mk, refs = D.batch_reference(shape)
    B, (_, _, _, _, res) = resident(shape)
    B.select_defect(source, medfilt)
    d, bo, cnt, km = B.download_defect(km=True)
    assert d.dtype == bo.dtype == km.dtype == np.uint8 and cnt.dtype == np.int64
    for q, r in enumerate(refs):
        rd, rbo = D.filtered(r["raw"][source], medfilt)
        assert np.array_equal(d[q], rd), q
        assert np.array_equal(bo[q], rbo), q
        assert cnt[q] == int(rd.sum()), (q, cnt[q], int(rd.sum()))
        assert np.array_equal(km[q], r["km"]), q
        if medfilt == 0 and source == "lb":
            assert cnt[q] == res[q].n_lb12 == r["n_lb12"], q
        if medfilt == 0 and source == "kmeans":
            assert cnt[q] == res[q].n_km0 == r["n_km0"], q
    assert not d[2].any() and not bo[2].any() and not km[2].any() and cnt[2] == 0   # the empty mask
    _, d2, bo2, _, _ = B.download()   # download() sees the selected maps too
    assert np.array_equal(d2, d) and np.array_equal(bo2, bo)


@pytest.mark.parametrize("shape", [(41, 37, 9), (40, 24, 1)], ids=str)
def test_mean_reproduces_the_run(shape):
    hp, mk, _ = D.batch_reference(shape)
    B = _lib.Batch(*shape, hp.shape[0])
    B.upload(hp, mk)
    B.run(B.options(do_n4=False, vox=VOX))
    first = B.download()
    assert first[1].any()
    B.select_defect("kmeans")
    after = B.download()
    assert not np.array_equal(after[1], first[1])          # the maps are the selection's now ...
    assert np.array_equal(after[3], first[3])              # ... the LB class volume is not touched
    for ra, rb in zip(first[4], after[4]):                 # ... and the run's results stay
        for name, _ in _lib.VdpResult._fields_:
            a, b = getattr(ra, name), getattr(rb, name)
            assert (list(a) == list(b)) if hasattr(a, "__len__") else (a == b or (a != a and b != b)), name
    B.select_defect("mean", 1)
    d, bo, cnt = B.download_defect()
    assert np.array_equal(d, first[1]) and np.array_equal(bo, first[2])
    assert list(cnt) == [r.n_defect for r in first[4]]
    B.select_defect("lb", 0)
    B.run(B.options(do_n4=False, vox=VOX))                 # a run restores the mean-anchored maps
    again = B.download()
    assert np.array_equal(again[1], first[1]) and np.array_equal(again[2], first[2])
    B.run(B.options(do_n4=False, vox=VOX, morph3d=True))
    m3 = B.download()
    B.select_defect("lb", 1)
    B.select_defect("mean", 2)
    d, bo, cnt = B.download_defect()
    assert np.array_equal(d, m3[1]) and np.array_equal(bo, m3[2])
    assert list(cnt) == [r.n_defect for r in m3[4]]
    B.close()


@pytest.mark.parametrize("shape", D.SHAPES, ids=str)
def test_km_cuts(shape):
    _, _, refs = D.batch_reference(shape)
    B, _ = resident(shape)
    cuts = B.km_cuts()
    assert cuts.dtype == np.float32 and cuts.shape == (len(refs), 3)
    for q, r in enumerate(refs):
        assert np.array_equal(cuts[q], r["cuts"]), (q, cuts[q], r["cuts"])


def test_cuts_from_the_large_volume_kmeans(monkeypatch):
    """k_kmeans (the kernel of volumes past 512 Ki voxels, forced here by VH_KM_OLD) stores the same
    cuts as k_kmeans_s: labels, cut values and the k-means map equal the reference."""
    shape = (41, 37, 9)
    hp, mk, refs = D.batch_reference(shape)
    monkeypatch.setenv("VH_KM_OLD", "1")
    B = _lib.Batch(*shape, hp.shape[0])
    B.upload(hp, mk)
    B.run(B.options(do_n4=False, vox=VOX))
    B.select_defect("kmeans", 0)
    d, _, cnt, km = B.download_defect(km=True)
    cuts = B.km_cuts()
    B.close()
    for q, r in enumerate(refs):
        assert np.array_equal(km[q], r["km"]) and np.array_equal(d[q], r["raw"]["kmeans"]), q
        assert cnt[q] == r["n_km0"] and np.array_equal(cuts[q], r["cuts"]), q


def oracle_ci(d, Rmax):
    """(shell int16, scalar, status) of one study as download_ci reports them (shell None where
    the oracle raises), as tests/test_gpu_ci_batch.py forms them."""
    d = np.asarray(d) != 0
    if not d.any():
        return np.full(d.shape, -1, np.int16), np.nan, _lib.VH_ERR_EMPTY
    table = compact_table_for(VOX, Rmax, d.shape)
    try:
        ref, shell = native.ci(d, table, VOX)
    except ValueError:
        return None, np.nan, _lib.VH_ERR_MAXRADIUS
    return shell.astype(np.int16), O.ci_scalar(ref[d]), _lib.VH_OK


@pytest.mark.parametrize("form", [None, "2"], ids=["auto", "form2"])
@pytest.mark.parametrize("source,medfilt", [("lb", 0), ("kmeans", 1)])
@pytest.mark.parametrize("shape", [(41, 37, 9), (40, 24, 1)], ids=str)
def test_ci_of_the_selection(shape, source, medfilt, form, monkeypatch):
    """Batch.ci after a selection is the oracle's CI of the reference map: shells, scalar, status."""
    if form is None:
        monkeypatch.delenv("VH_CI_FORM", raising=False)
    else:
        monkeypatch.setenv("VH_CI_FORM", form)
    _, _, refs = D.batch_reference(shape)
    B, _ = resident(shape)
    B.select_defect(source, medfilt)
    B.ci(VOX, 12)
    sh, sc, status = B.download_ci(maps="shell")
    for q in (0, 1, 2):   # the two fields and the empty study
        rsh, rsc, rst = oracle_ci(D.filtered(refs[q]["raw"][source], medfilt)[0], 12)
        assert status[q] == rst, (q, status[q], rst)
        if rst == _lib.VH_OK:
            assert sc[q] == rsc, (q, sc[q], rsc)
        else:
            assert np.isnan(sc[q]), (q, sc[q])
        if rsh is not None:
            assert np.array_equal(sh[q], rsh), q
    assert status[0] == _lib.VH_OK   # (the seed-1 field's maps are walkable at Rmax 12)


def test_with_n4_on_a_golden_case(cases):
    """One 128x128x16 golden case.  The goldens were made with N4 = identity (make_goldens.py), so
    with do_n4 = 0 MEAN / medfilt 1 is the golden defect map and border and LB / 0 the golden LB
    classes 1 and 2.  With N4 on the selection reads the run's N4 volume, not HPvent: the same two
    selections equal the run's own maps and the oracle chain on the downloaded N4."""
    X, M, vox, exp, name = next(c for c in cases if c[0].shape == (128, 128, 16))
    B = _lib.Batch(128, 128, 16, 1)
    B.upload(X[None].astype(np.float32), M[None].astype(np.uint8))
    for do_n4 in (False, True):
        B.run(B.options(do_n4=do_n4, vox=vox))
        n4, rd, rbo, rlb, _ = B.download(n4=True)
        if do_n4:
            assert not np.array_equal(n4[0], X.astype(np.float32))
            o = O.calculate_vdp(n4[0], M, vox)
            want = (o["defectArray"], o["defectBorder"], np.isin(o["defectArrayLB"], (1, 2)))
        else:
            want = (exp["defect"], exp["defect_border"], np.isin(exp["lb"], (1, 2)))
        B.select_defect("lb", 0)
        d, _, cnt = B.download_defect()
        assert np.array_equal(d[0] != 0, want[2]) and np.array_equal(d[0] != 0, np.isin(rlb[0], (1, 2))), name
        assert cnt[0] == int(want[2].sum())
        B.select_defect("mean", 1)
        d, bo, cnt = B.download_defect()
        assert np.array_equal(d[0], want[0]) and np.array_equal(d[0], rd[0]), name
        assert np.array_equal(bo[0] != 0, want[1]) and np.array_equal(bo[0], rbo[0]), name
        assert cnt[0] == int(want[0].sum())
    B.close()


def test_host_buffer_form_equals_the_batch():
    shape = (41, 37, 9)
    hp, mk, refs = D.batch_reference(shape)
    B, _ = resident(shape)
    keep = [0, 1, 3, 4]   # (vh_defect_map raises for an empty-mask study, like vh_vdp)
    for source in D.SOURCES:
        B.select_defect(source, 1)
        d, bo, cnt, km = B.download_defect(km=True)
        hd, hbo, hcnt, hkm = _lib.defect_map(hp[keep], mk[keep], source, km=True)
        assert np.array_equal(hd, d[keep]) and np.array_equal(hbo, bo[keep])
        assert np.array_equal(hcnt, cnt[keep]) and np.array_equal(hkm, km[keep])
        one = _lib.defect_map(hp[0], mk[0], source, medfilt=0)   # a single volume, no labels
        assert len(one) == 3 and np.array_equal(one[0][0], refs[0]["raw"][source])
    with pytest.raises(IndexError):
        _lib.defect_map(hp[2], mk[2], "lb")


def identity_n4(hp, mask):
    return np.asarray(hp, dtype=np.float32).copy()


def test_class_select_defect():
    from vent_analysis_amd import Vent_Analysis
    shape = (66, 66, 2)   # (rows enough for calculate_SNR's noise band)
    hp, mk, refs = D.batch_reference(shape)
    va = Vent_Analysis(xenon_array=hp[0].copy(), mask_array=mk[0].astype(np.float64), vox=VOX)
    va.N4_bias_correction = identity_n4   # (the class's documented caller-supplied N4)
    va.calculate_VDP()
    meta = copy.deepcopy(va.metadata)
    lb_before = va.defectArrayLB.copy()
    attrs = set(vars(va))
    pct = va.select_defect("kmeans")
    rd, rbo = D.filtered(refs[0]["raw"]["kmeans"], 1)
    assert pct == 100 * np.float64(rd.sum()) / np.sum(mk[0].astype(np.float64))
    assert va.defectArray.dtype == np.float64 and np.array_equal(va.defectArray, rd)
    assert np.array_equal(va.defectBorder, rbo == 1)
    np.testing.assert_equal(va.metadata, meta)
    assert np.array_equal(va.defectArrayLB, lb_before)
    assert set(vars(va)) == attrs   # no new attribute
    va.calculate_CI()
    table = compact_table_for(VOX, 50, shape)
    ref, _ = native.ci(rd != 0, table, VOX)
    assert np.array_equal(va.CIarray, ref) and va.metadata["CI"] == O.ci_scalar(ref[rd != 0])
    assert va.build4DdataArray()[..., 4].sum() == rd.sum()


def test_class_scales_by_the_mask_value():
    """A 0/255 mask: defectArray is the map times 255, as calculate_VDP scales its own."""
    from vent_analysis_amd import Vent_Analysis
    shape = (66, 66, 2)
    hp, mk, refs = D.batch_reference(shape)
    m255 = mk[0].astype(np.float64) * 255
    va = Vent_Analysis(xenon_array=hp[0].copy(), mask_array=m255, vox=VOX)
    va.calculate_VDP()
    assert np.array_equal(np.unique(va.defectArray), [0.0, 255.0])
    pct = va.select_defect("lb", medfilt=0)
    assert np.array_equal(va.defectArray, refs[0]["raw"]["lb"] * 255.0)
    assert pct == 100 * np.sum(va.defectArray) / np.sum(m255)
    assert np.array_equal(va.defectBorder, D.filtered(refs[0]["raw"]["lb"], 0)[1] == 1)


def test_no_plane_geometry_is_a_clean_error(monkeypatch):
    """Where the plane sweep is not available (here: switched off, as for a shape it cannot take)
    the selection refuses with ValueError and leaves the run's maps as they were."""
    shape = (33, 20, 5)
    hp, mk, _ = D.batch_reference(shape)
    B = _lib.Batch(*shape, hp.shape[0])
    B.upload(hp, mk)
    monkeypatch.setenv("VH_CLASSIFY_TILE", "1")
    B.run(B.options(do_n4=False, vox=VOX))
    before = B.download()
    with pytest.raises(ValueError):
        B.select_defect("lb", 0)
    d, bo, cnt = B.download_defect()
    assert np.array_equal(d, before[1]) and np.array_equal(bo, before[2])
    assert list(cnt) == [r.n_defect for r in before[4]]
    monkeypatch.delenv("VH_CLASSIFY_TILE")
    B.select_defect("lb", 0)                 # the batch still works
    assert list(B.download_defect()[2]) == [r.n_lb12 for r in before[4]]
    B.close()


def test_argument_errors():
    shape = (7, 5, 3)
    hp, mk, refs = D.batch_reference(shape)
    B = _lib.Batch(*shape, hp.shape[0])
    B.upload(hp, mk)
    with pytest.raises(ValueError):
        B.select_defect("mean")              # before any run
    with pytest.raises(ValueError):
        B.download_defect()
    with pytest.raises(ValueError):
        B.km_cuts()
    B.run(B.options(do_n4=False, do_kmeans=False, vox=VOX))
    for bad in (dict(source=3), dict(source=-1), dict(source="km"), dict(source="lb", medfilt=3),
                dict(source="lb", medfilt=-1), dict(source="kmeans")):   # no k-means in that run
        with pytest.raises(ValueError):
            B.select_defect(**bad)
    with pytest.raises(ValueError):
        B.download_defect(km=True)
    with pytest.raises(ValueError):
        B.km_cuts()
    B.select_defect("lb", 0)                 # the batch still works
    d, bo, cnt = B.download_defect()
    assert all(np.array_equal(d[q], refs[q]["raw"]["lb"]) for q in range(len(refs)))
    B.run(B.options(do_n4=False, vox=VOX))
    B.select_defect("kmeans", 0)
    d, bo, cnt = B.download_defect()
    assert all(np.array_equal(d[q], refs[q]["raw"]["kmeans"]) for q in range(len(refs)))
    B.close()
