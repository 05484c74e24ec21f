"""GPU: the regional analysis of a resident batch (vh_batch_zones / Batch.zones and the layers above
it) against the numpy reference (zones_ref).  Everything is an integer: every comparison is exact,
over every study.

The byte model of the "zones_b" timing class, per voxel of the batch: the profile sweep reads the mask
(1); the map pass reads the mask and writes the zone (2), and with labels also reads the label (3); the
count sweep reads N4 (4), mask, defect, LB class and zone (1 each: 8).  11 bytes geometric, 12 with
labels; the profiles, tables and counts are not counted."""
import copy
import functools
import itertools

import numpy as np
import pytest

from vent_analysis_amd import _lib

import distribution_ref as DR
import zones_ref as R

pytestmark = pytest.mark.gpu

VOX = R.VOX
PARTS = [((1, 1, 1), False), ((3, 1, 1), True), ((2, 3, 2), False), ((32, 1, 1), False), ((3, 1, 2), True)]
BYS = ("extent", "count")
NORMS = ("mean", "p99")
BINS_HI = ((100, 1.5), (1, 0.5), (256, 2.0), (7, 64.0))
# every third of the 80 combinations, the shapes in turn: every shape and every parameter value is in
COMBOS = list(itertools.product(PARTS, BYS, NORMS, BINS_HI))[::3]
CASES = [(R.SHAPES[n % len(R.SHAPES)],) + c for n, c in enumerate(COMBOS)]


def case_id(v):
    return str(v).replace(" ", "")


def test_the_cases_cover_every_value():
    assert {c[0] for c in CASES} == set(R.SHAPES) and {c[1] for c in CASES} == set(PARTS)
    assert {c[2] for c in CASES} == set(BYS) and {c[3] for c in CASES} == set(NORMS)
    assert {c[4] for c in CASES} == set(BINS_HI)


def plain_run(shape, **kw):
    hp, mk = R.batch_inputs(shape)
    B = _lib.Batch(*shape, hp.shape[0])
    B.upload(hp, mk)
    B.run(B.options(do_n4=False, do_snr=False, vox=VOX, **kw))
    return B


@functools.lru_cache(maxsize=None)
def resident(shape):
    """The batch of a shape after one plain run (N4 = identity, no SNR), kept resident for the
    parametrised cases, with the run's defect map and LB classes: the maps the sweep reads."""
    B = plain_run(shape)
    _, d, _, lb, _ = B.download()
    d.setflags(write=False)
    lb.setflags(write=False)
    return B, d, lb


def references(shape, defect, lb, **kw):
    hp, mk = R.batch_inputs(shape)
    return [R.reference(hp[q], mk[q], defect[q], lb[q], **kw) for q in range(hp.shape[0])]


def check_derived(got, K, bins, hi):
    nb = got["counts"].shape[0]
    assert got["n_zones"] == K and got["counts"].shape == (nb, K + 1, _lib.VH_ZONE_COLS)
    assert got["hist"].shape == (nb, K + 1, bins) and got["stats"].shape == (nb, K + 1, 4)
    assert got["geom"].shape == (nb, 8) and got["geom"].dtype == np.int32
    assert np.array_equal(got["edges"], np.arange(bins + 1) * (hi / bins)) and got["edges"].dtype == np.float64
    assert np.array_equal(got["zone_vdp"], _lib.zone_vdp(got["counts"]), equal_nan=True)
    assert np.array_equal(got["zone_mean"], _lib.zone_mean(got["stats"]), equal_nan=True)


@pytest.mark.parametrize("shape", [(41, 37, 9), (7, 5, 3)], ids=str)
def test_the_run_leaves_the_references_inputs(shape):
    """The run's defect map and LB class volume, which the cases below hand to the reference, are the
    numpy ones."""
    defect, lb = R.batch_maps(shape)
    _, d, l = resident(shape)
    assert np.array_equal(d, defect) and np.array_equal(l, lb)


@pytest.mark.parametrize("shape,pl,by,norm,bh", CASES, ids=case_id)
def test_geometric_zones_equal_the_reference(shape, pl, by, norm, bh):
    (parts, lateral), (bins, hi) = pl, bh
    B, d, lb = resident(shape)
    B.zones(parts, lateral, by, norm=norm, bins=bins, hi=hi)
    got = B.download_zones()
    K = R.n_zones(parts, lateral)
    check_derived(got, K, bins, hi)
    refs = references(shape, d, lb, parts=parts, lateral=lateral, by=BYS.index(by), norm=norm, bins=bins, hi=hi)
    R.assert_equal(got, refs)
    assert not got["map"][2].any() and not got["counts"][2].any() and not got["hist"][2].any()   # the empty mask
    assert not got["counts"][:, 0].any() and not got["hist"][:, 0].any()                          # zone 0: nothing
    if lateral:
        mk = R.batch_inputs(shape)[1]
        assert not mk[0][:, got["geom"][0, 6], :].any()        # the clear gap: an empty column between the lungs
        assert got["geom"][4, 6] == shape[1] // 2              # the single column: s = lo, side 0 is empty
    else:
        assert (got["geom"][:, 6] == -1).all()
    counts = B.download_zones(map=False)
    assert counts["map"] is None
    R.assert_equal(counts, refs, ("counts", "hist", "stats", "geom"))


def test_labels_mode():
    """Bytes 0..40 at K = 5: zero and out-of-range labels land in zone 0, labels off the mask count
    nothing; then K = 32; then the geometric map as labels gives the geometric result."""
    shape = (41, 37, 9)
    hp, mk = R.batch_inputs(shape)
    B, d, lb = resident(shape)
    labels = np.random.default_rng(8).integers(0, 41, hp.shape).astype(np.uint8)
    for K, norm, bins, hi in ((5, "mean", 100, 1.5), (32, "p99", 7, 2.0)):
        B.zones(labels=labels, n_zones=K, norm=norm, bins=bins, hi=hi)
        got = B.download_zones()
        check_derived(got, K, bins, hi)
        refs = [R.reference(hp[q], mk[q], d[q], lb[q], labels=labels[q], K=K, norm=norm, bins=bins, hi=hi)
                for q in range(hp.shape[0])]
        R.assert_equal(got, refs)
        assert (got["geom"][:, 6] == -1).all() and got["counts"][0, 0, 0] > 0
        assert np.array_equal(got["counts"][:, :, 0].sum(axis=1), (mk != 0).sum(axis=(1, 2, 3)))
        assert not got["map"][mk == 0].any() and got["map"].max() == K
    with pytest.raises(ValueError):
        B.zones(labels=labels)               # n_zones None is the largest label: 40 is refused
    B.zones((3, 1, 2), True, "count", norm="mean", bins=100, hi=1.5)
    geo = B.download_zones()
    B.zones(labels=np.array(geo["map"]), n_zones=geo["n_zones"], norm="mean", bins=100, hi=1.5)
    lab = B.download_zones()
    for k in ("map", "counts", "hist", "stats"):
        assert np.array_equal(geo[k], lab[k]), k
    assert np.array_equal(geo["geom"][:, :6], lab["geom"][:, :6]) and (lab["geom"][:, 6] == -1).all()


@pytest.mark.parametrize("norm,bins,hi", [("mean", 100, 1.5), ("p99", 256, 2.0)])
def test_zone_sums_equal_the_other_analyses(norm, bins, hi):
    """On the device: summed over zones the histogram and the below / over counts are the
    distribution's, the class columns its slice counts', the defect column core_rind's total."""
    shape = (33, 20, 5)
    _, mk = R.batch_inputs(shape)
    B, _, _ = resident(shape)
    B.distribution(norm, bins, hi)
    dist = B.download_distribution()
    B.core_rind(thresholds=(3,))
    cr = B.download_core_rind(map=False)
    for kw in (dict(parts=(3, 1, 2), lateral=True), dict(parts=(2, 3, 2), lateral=False, by="count")):
        B.zones(norm=norm, bins=bins, hi=hi, **kw)
        got = B.download_zones(map=False)
        assert np.array_equal(got["hist"].sum(axis=1, dtype=np.uint32), dist["hist"])
        assert np.array_equal(got["stats"][:, :, 1:3].sum(axis=1), dist["outside"])
        assert np.array_equal(got["counts"][:, :, 2:].sum(axis=1), dist["slice_counts"][:, :, 2:].sum(axis=1))
        assert np.array_equal(got["counts"][:, :, 0].sum(axis=1), dist["slice_counts"][:, :, 0].sum(axis=1))
        assert np.array_equal(got["counts"][:, :, 1].sum(axis=1), cr["counts"][:, :, 1].sum(axis=1))
        assert got["counts"][:, :, 0].sum() == int((mk != 0).sum()) > 0


def test_the_defect_column_follows_the_resident_map():
    shape = (41, 37, 9)
    hp, mk = R.batch_inputs(shape)
    B = plain_run(shape)
    _, d0, _, lb, res = B.download()
    kw = dict(parts=(3, 1, 1), lateral=True, by=R.EXTENT, norm="mean", bins=100, hi=1.5)
    B.zones()
    got = B.download_zones()
    R.assert_equal(got, references(shape, d0, lb, **kw))
    # a plain run: n_defect counts the whole map, and the median can set a voxel next to the mask
    off = ((d0 != 0) & (mk == 0)).sum(axis=(1, 2, 3))
    assert list(got["counts"][:, :, 1].sum(axis=1) + off) == [r.n_defect for r in res] and off.sum() < 10
    B.select_defect("lb", 0)
    B.zones()
    got = B.download_zones()
    d1, _, cnt = B.download_defect()
    assert np.array_equal(got["counts"][:, :, 1].sum(axis=1), cnt) and cnt[0] != res[0].n_defect
    R.assert_equal(got, references(shape, d1, lb, **kw))
    up = (np.random.default_rng(9).random(hp.shape) < 0.2).astype(np.uint8) * 3   # off-mask voxels too
    B.upload_defect(up)
    B.zones()
    got = B.download_zones()
    R.assert_equal(got, references(shape, up, lb, **kw))
    assert np.array_equal(got["counts"][:, :, 1].sum(axis=1), ((up != 0) & (mk != 0)).sum(axis=(1, 2, 3)))
    assert not got["counts"][2].any()       # the empty mask: the uploaded defects off the mask count nothing
    B.close()


def test_lifecycle():
    shape = (7, 5, 3)
    hp, mk = R.batch_inputs(shape)
    B = _lib.Batch(*shape, hp.shape[0])
    B.upload(hp, mk)
    with pytest.raises(ValueError):
        B.zones()                            # before any run
    with pytest.raises(ValueError):
        B.download_zones()
    opts = B.options(do_n4=False, do_snr=False, vox=VOX)
    B.run(opts)
    _, d, _, lb, _ = B.download()
    with pytest.raises(ValueError):
        B.download_zones()                   # nothing enqueued yet
    B.zones()
    R.assert_equal(B.download_zones(), references(shape, d, lb))
    B.zones((2, 3, 2), False, "count", norm="p99", bins=7, hi=2.0)       # a second call: new K and bins
    B.zones((1, 1, 1), False, norm="p99", bins=3, hi=2.0)                # enqueued behind it, not downloaded between
    got = B.download_zones()
    assert got["counts"].shape[1] == 2 and got["hist"].shape[1:] == (2, 3)
    R.assert_equal(got, references(shape, d, lb, parts=(1, 1, 1), lateral=False, norm="p99", bins=3, hi=2.0))
    B.zones((2, 3, 2), False, "count", norm="p99", bins=7, hi=2.0)
    got = B.download_zones()
    assert got["counts"].shape[1] == 13 and got["hist"].shape[1:] == (13, 7)
    R.assert_equal(got, references(shape, d, lb, parts=(2, 3, 2), lateral=False, by=R.COUNT, norm="p99", bins=7, hi=2.0))
    B.run(opts)
    with pytest.raises(ValueError):
        B.download_zones()                   # the run discarded it
    B.zones()
    B.edit_mask("dilate", 1)
    with pytest.raises(ValueError):
        B.download_zones()                   # so did the edit
    with pytest.raises(ValueError):
        B.zones()                            # which forgot the run
    B.run(opts)
    B.zones()
    B.denoise(sigma=0.05)
    with pytest.raises(ValueError):
        B.download_zones()
    B.upload(hp, mk)
    B.run(opts)
    B.zones()                                # the batch still works
    R.assert_equal(B.download_zones(), references(shape, d, lb))
    B.close()


def test_read_only():
    shape = (41, 37, 9)
    hp, mk = R.batch_inputs(shape)
    B = plain_run(shape, do_kmeans=False)
    B.distribution("mean", 64, 1.5)
    B.core_rind(thresholds=(3, 13))

    def snapshot():
        n4, d, bo, lb, res = B.download(n4=True)
        dd = B.download_defect()
        ds = B.download_distribution()
        cr = B.download_core_rind()
        return ([a.tobytes() for a in (n4, d, bo, lb)] + [bytes(r) for r in res] + [a.tobytes() for a in dd]
                + [B.download_mask().tobytes()] + [ds[k].tobytes() for k in ("hist", "outside", "slice_counts")]
                + [cr[k].tobytes() for k in ("d2", "counts", "stats")])

    before = snapshot()
    B.zones()
    first = B.download_zones()
    assert snapshot() == before
    labels = np.random.default_rng(4).integers(0, 9, hp.shape).astype(np.uint8)
    B.zones(labels=labels, n_zones=8, norm="p99", bins=256, hi=2.0)
    B.download_zones()
    assert snapshot() == before
    B.zones()                                # and the sweep itself is deterministic
    second = B.download_zones()
    assert all(np.array_equal(first[k], second[k], equal_nan=True) for k in first)
    B.close()


def test_library_argument_errors():
    """The library's own checks (the binding's are bypassed): VH_ERR_ARG, nothing enqueued -- the
    result of the valid call before them is what a later download returns."""
    shape = (7, 5, 3)
    hp, mk = R.batch_inputs(shape)
    B = plain_run(shape)
    _, d, _, lb, _ = B.download()
    labels = np.ones(hp.shape, np.uint8)

    def call(parts=(3, 1, 1), lateral=1, by=0, norm=0, bins=100, hi=1.5, lab=None, n_zones=0):
        p = None if parts is None else np.asarray(parts, np.int32)
        return B.L.vh_batch_zones(B.h, _lib._ptr(lab), n_zones, _lib._ptr(p), lateral, by, norm, bins, _lib.ct.c_float(hi))

    B.zones((2, 1, 2), True, "count", norm="p99", bins=7, hi=2.0)
    for bad in (dict(norm=2), dict(norm=-1), dict(bins=0), dict(bins=257), dict(hi=0.0), dict(hi=-1.0),
                dict(hi=float("inf")), dict(hi=float("nan")), dict(hi=64.5), dict(by=2), dict(by=-1),
                dict(parts=(0, 1, 1)), dict(parts=(3, 1, -2)), dict(parts=None), dict(parts=(17, 1, 1)),
                dict(parts=(3, 4, 3), lateral=0), dict(parts=(33, 1, 1), lateral=0), dict(lateral=2), dict(lateral=-1),
                dict(parts=(3, 2, 1)), dict(lab=labels, n_zones=0), dict(lab=labels, n_zones=33),
                dict(lab=labels, n_zones=-1)):
        assert call(**bad) == _lib.VH_ERR_ARG, bad
    with pytest.raises(ValueError):
        B.ctx.check(call(bins=0), "vh_batch_zones")
    R.assert_equal(B.download_zones(), references(shape, d, lb, parts=(2, 1, 2), lateral=True, by=R.COUNT, norm="p99",
                                                  bins=7, hi=2.0))
    assert call(hi=64.0, bins=256, parts=(4, 1, 4)) == _lib.VH_OK     # the limits themselves are inside
    assert call(lab=labels, n_zones=32, parts=None, lateral=9, by=9) == _lib.VH_OK   # geometry not looked at
    B.close()


def identity_n4(hp, mask):
    return np.asarray(hp, dtype=np.float32).copy()


def test_host_buffer_form_and_the_class():
    from vent_analysis_amd import Vent_Analysis
    shape = (66, 66, 2)
    X, _ = DR.D.field(shape, 1)
    M = R.lungs(shape)
    defect, lb = DR.run_defect(X, M), DR.lb_volume(X, M)
    up = (np.random.default_rng(2).random(shape) < 0.3).astype(np.uint8)
    for kw, df in ((dict(), None), (dict(parts=(3, 1, 2), lateral=True, by="count", norm="p99", bins=7, hi=2.0), up)):
        got = _lib.zones(X, M, df, **kw)
        ref = R.reference(X, M, defect if df is None else df, lb, **{**kw, "by": BYS.index(kw.get("by", "extent"))})
        R.assert_equal(got, [ref])
    lab = np.random.default_rng(6).integers(0, 7, shape).astype(np.uint8)
    got = _lib.zones(X, M, labels=lab, n_zones=4, map=False)
    assert got["map"] is None
    R.assert_equal(got, [R.reference(X, M, defect, lb, labels=lab, K=4)], ("counts", "hist", "stats", "geom"))
    with pytest.raises(IndexError):
        _lib.zones(X, np.zeros(shape, np.uint8))
    with pytest.raises(ValueError):
        _lib.zones(X, M, bins=0)

    _, M = DR.D.field(shape, 1)              # one ellipse: the median sets no voxel off this mask (checked below)
    va = Vent_Analysis(xenon_array=X.copy(), mask_array=M.astype(np.float64), vox=VOX)
    va.N4_bias_correction = identity_n4
    va.calculate_VDP()
    meta = copy.deepcopy(va.metadata)
    before = {k: v.tobytes() for k, v in vars(va).items() if isinstance(v, np.ndarray)}
    attrs = set(vars(va))
    out = va.regional_vdp()
    ref = R.reference(va.N4HPvent, va.mask, va.defectArray, va.defectArrayLB)
    for k in ("map", "counts", "hist", "stats", "geom"):
        assert out[k].dtype == ref[k].dtype and np.array_equal(out[k], ref[k]), k
    assert out["n_zones"] == 6 and out["zone_vdp"].shape == (7,) and out["edges"].shape == (101,)
    c = out["counts"]
    n = np.float64(c[:, 0].sum())
    assert not va.defectArray[va.mask == 0].any()
    assert 100 * np.float64(c[:, 1].sum()) / n == va.metadata["VDP"]            # the zones recombine
    assert c[:, 1].sum() == int(va.defectArray.sum()) and c[:, 0].sum() == int((va.mask != 0).sum())
    assert 100 * np.float64(c[:, 2:4].sum()) / n == va.metadata["VDP_lb"]
    on = c[:, 0] > 0
    assert on[1:].all() and np.array_equal(out["zone_vdp"][on], 100 * c[on, 1] / c[on, 0])
    out2 = va.regional_vdp(labels=lab, n_zones=4, norm="p99", bins=7, hi=2.0)
    ref2 = R.reference(va.N4HPvent, va.mask, va.defectArray, va.defectArrayLB, labels=lab, K=4, norm="p99", bins=7, hi=2.0)
    for k in ("map", "counts", "hist", "stats", "geom"):
        assert np.array_equal(out2[k], ref2[k]), k
    np.testing.assert_equal(va.metadata, meta)                                 # no metadata key, no attribute
    assert set(vars(va)) == attrs
    assert {k: v.tobytes() for k, v in vars(va).items() if isinstance(v, np.ndarray)} == before


def test_kernel_time():
    shape = (33, 20, 5)
    hp, _ = R.batch_inputs(shape)
    B = plain_run(shape, profile=True)
    B.zones()
    B.zones((2, 3, 2), False, "count", norm="p99", bins=10, hi=2.0)
    B.download_zones()
    ms, launches, nbytes = B.kernel_time("zones_b")
    assert launches == 2 and ms > 0
    assert nbytes == 11.0 * B.shape[0] * np.prod(shape)
    B.zones(labels=np.ones(hp.shape, np.uint8), n_zones=1)
    B.download_zones()
    ms, launches, nbytes = B.kernel_time("zones_b")
    B.close()
    assert launches == 3 and nbytes == 12.0 * B.shape[0] * np.prod(shape)
