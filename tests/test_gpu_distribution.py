"""GPU: the ventilation distribution of a resident batch (vh_batch_distribution / Batch.distribution
and the layers above it) against the numpy reference (distribution_ref).  Everything is an integer
count: every comparison is exact."""
import copy
import functools

import numpy as np
import pytest

from vent_analysis_amd import _lib

import batch_render_ref as BR
import distribution_ref as R

pytestmark = pytest.mark.gpu

VOX = R.VOX
ALL_SHAPES = R.SHAPES + [R.TALL]


def plain_run(shape, **kw):
    hp, mk, _, _ = R.batch_inputs(shape)
    B = _lib.Batch(*shape, hp.shape[0])
    B.upload(hp, mk)
    B.run(B.options(do_n4=False, do_snr=False, vox=VOX, **kw))
    return B


@functools.lru_cache(maxsize=None)
def resident(shape):
    """The batch of a shape after one plain run (N4 = identity, no SNR), kept resident for the
    parametrised cases, and that run's download."""
    B = plain_run(shape)
    return B, B.download()


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=str)
def test_the_run_leaves_the_references_inputs(shape):
    """The maps the sweep reads are the ones the reference counts: the run's defect map and LB class
    volume equal the oracle's, the all-zero study (NaN classes) included."""
    _, _, defect, lb = R.batch_inputs(shape)
    _, (_, d, _, l, _) = resident(shape)
    assert np.array_equal(d, defect) and np.array_equal(l, lb)


@pytest.mark.parametrize("bins,hi", R.PARAMS)
@pytest.mark.parametrize("norm", R.NORMS)
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=str)
def test_distribution_equals_the_reference(shape, norm, bins, hi):
    B, _ = resident(shape)
    B.distribution(norm, bins, hi)
    got = B.download_distribution()
    nb = B.shape[0]
    assert got["hist"].shape == (nb, bins) and got["outside"].shape == (nb, 2)
    assert got["slice_counts"].shape == (nb, shape[2], _lib.VH_DIST_COLS)
    assert np.array_equal(got["edges"], np.arange(bins + 1) * (hi / bins)) and got["edges"].dtype == np.float64
    R.assert_equal(got, R.batch_reference(shape, norm, bins, hi))
    assert not got["hist"][2].any() and not got["outside"][2].any() and not got["slice_counts"][2].any()


def test_p99_rows_sum_to_the_cohort():
    shape = (41, 37, 9)
    B = plain_run(shape, do_cohort=True)
    B.distribution("p99", _lib.COHORT_BINS, 1.5)
    hist = B.download_distribution()["hist"]
    cohort = B.cohort_hist()
    B.close()
    assert cohort.sum() > 0 and np.array_equal(hist.sum(axis=0, dtype=np.uint64), cohort)


def test_counts_follow_the_resident_defect_map():
    shape = (41, 37, 9)
    hp, mk, defect, lb = R.batch_inputs(shape)
    B = plain_run(shape)
    res = B.download()[4]
    B.distribution()
    sl = B.download_distribution()["slice_counts"]
    assert list(sl[:, :, 1].sum(axis=1)) == [r.n_defect for r in res]      # a plain run
    assert list(sl[:, :, 0].sum(axis=1)) == [r.n_mask for r in res]
    B.select_defect("lb", 0)
    B.distribution("mean", 100, 1.5)
    got = B.download_distribution()
    d, _, cnt = B.download_defect()
    sl = got["slice_counts"]
    assert np.array_equal(sl[:, :, 1].sum(axis=1), cnt) and cnt[0] != res[0].n_defect
    assert list(sl[:, :, 2:4].sum(axis=(1, 2))) == [r.n_lb12 for r in res] == list(cnt)
    refs = R.batch_reference(shape, "mean", 100, 1.5)
    for q in range(hp.shape[0]):   # the histogram does not depend on the map; the slice counts follow it
        assert np.array_equal(got["hist"][q], refs[q]["hist"]), q
        assert np.array_equal(sl[q], R.slice_counts(mk[q], d[q], lb[q])), q
    up = (np.random.default_rng(9).random(hp.shape) < 0.2).astype(np.uint8) * 3   # off-mask voxels too
    B.upload_defect(up)
    B.distribution("mean", 100, 1.5)
    sl = B.download_distribution()["slice_counts"]
    for q in range(hp.shape[0]):
        assert np.array_equal(sl[q], R.slice_counts(mk[q], up[q], lb[q])), q
    assert sl[2, :, 1].sum() == int((up[2] != 0).sum()) > 0 and not sl[2, :, 0].any()   # the empty mask
    B.close()


def test_an_uploaded_map_counts_by_nonzero_bytes():
    """Every byte 255, off the mask too: the defect column is the slice's voxel count, the class
    columns stay the run's."""
    shape = (7, 5, 3)
    hp, mk, _, lb = R.batch_inputs(shape)
    B = plain_run(shape)
    up = np.full(hp.shape, 255, np.uint8)
    B.upload_defect(up)
    B.distribution("p99", 7, 2.0)
    got = B.download_distribution()
    B.close()
    for q in range(hp.shape[0]):
        assert np.array_equal(got["slice_counts"][q], R.slice_counts(mk[q], up[q], lb[q])), q
    assert np.all(got["slice_counts"][:, :, 1] == shape[0] * shape[1])


def test_read_only():
    """download(), download_defect() and download_ci() return the same bytes before and after, and a
    montage drawn after it still shows the CI panel."""
    hp, mk, proton = BR.mixed_batch()
    B = _lib.Batch(*hp.shape[1:], hp.shape[0])
    B.upload(hp, mk)
    B.run(B.options(do_n4=False, vox=BR.VOX, do_cohort=True))
    pal = BR.parula()
    blank, _ = B.montage(pal, proton)
    B.select_defect("lb", 1)
    B.ci(BR.VOX, Rmax=12)

    def state():
        n4, d, bo, lb, res = B.download(n4=True)
        dd, bb, cnt, km = B.download_defect(km=True)
        scal = [(r.vdp, r.vdp_lb, r.vdp_km, r.n_mask, r.n_defect, r.n_lb12, r.mean_anchor, r.p99) for r in res]
        return [n4, d, bo, lb, dd, bb, cnt, km, B.km_cuts(), B.cohort_hist(), *B.download_ci("shell"),
                B.download_ci("f64")[0]], scal

    before, scal0 = state()
    with_ci, st0 = B.montage(pal, proton)
    B.distribution("p99", 1024, 1.5)
    first = B.download_distribution()
    B.distribution("mean", 100, 1.5)
    B.download_distribution()
    after, scal1 = state()
    assert repr(scal0) == repr(scal1)   # (NaN-safe)
    for x, y in zip(before, after):
        assert x.tobytes() == y.tobytes()
    again, st1 = B.montage(pal, proton)
    assert np.array_equal(st0, st1)
    shown = 0
    for a, b, c in zip(with_ci, again, blank):
        assert (a is None and b is None) or np.array_equal(a, b)
        shown += a is not None and not np.array_equal(a, c)
    assert shown >= 1   # the CI panel is drawn, before and after
    B.distribution("p99", 1024, 1.5)   # and the sweep itself is deterministic
    second = B.download_distribution()
    assert all(np.array_equal(first[k], second[k]) for k in first)
    B.close()


def test_a_second_call_replaces_the_first():
    shape = (33, 20, 5)
    B, _ = resident(shape)
    B.distribution("p99", 1024, 1.5)
    B.distribution("mean", 7, 2.0)          # enqueued behind it, not downloaded in between
    got = B.download_distribution()
    assert got["hist"].shape[1] == 7
    R.assert_equal(got, R.batch_reference(shape, "mean", 7, 2.0))
    B.distribution("p99", 1024, 1.5)
    R.assert_equal(B.download_distribution(), R.batch_reference(shape, "p99", 1024, 1.5))


def test_a_new_run_invalidates_and_argument_errors():
    shape = (7, 5, 3)
    hp, mk, _, _ = R.batch_inputs(shape)
    B = _lib.Batch(*shape, hp.shape[0])
    B.upload(hp, mk)
    with pytest.raises(ValueError):
        B.distribution()                     # before any run
    with pytest.raises(ValueError):
        B.download_distribution()
    B.run(B.options(do_n4=False, do_snr=False, vox=VOX))
    with pytest.raises(ValueError):
        B.download_distribution()            # nothing enqueued yet
    for bad in (dict(norm=2), dict(norm=-1), dict(norm="median"), dict(bins=0), dict(bins=1025), dict(bins=-3),
                dict(hi=0.0), dict(hi=-1.5), dict(hi=float("inf")), dict(hi=float("nan"))):
        with pytest.raises(ValueError):
            B.distribution(**bad)
    with pytest.raises(ValueError):
        B.download_distribution()            # a refused call enqueues nothing
    B.distribution("p99", 100, 1.5)
    R.assert_equal(B.download_distribution(), R.batch_reference(shape, "p99", 100, 1.5))
    with pytest.raises(ValueError):
        B.distribution(bins=2000)
    R.assert_equal(B.download_distribution(), R.batch_reference(shape, "p99", 100, 1.5))   # still the last one
    B.run(B.options(do_n4=False, do_snr=False, vox=VOX))
    with pytest.raises(ValueError):
        B.download_distribution()            # the run discarded it
    B.distribution("mean", 1, 0.5)           # the batch still works
    R.assert_equal(B.download_distribution(), R.batch_reference(shape, "mean", 1, 0.5))
    B.close()


def test_host_buffer_form():
    shape = (41, 37, 9)
    hp, mk, _, _ = R.batch_inputs(shape)
    keep = [0, 1, 3, 4, 5, 6]   # (vh_distribution raises for an empty-mask study, like vh_vdp)
    for norm, bins, hi in (("p99", 1024, 1.5), ("mean", 7, 2.0)):
        got = _lib.distribution(hp[keep], mk[keep], norm, bins, hi)
        refs = R.batch_reference(shape, norm, bins, hi)
        R.assert_equal(got, [refs[q] for q in keep])
        assert np.array_equal(got["edges"], np.arange(bins + 1) * (hi / bins))
    one = _lib.distribution(hp[0], mk[0], "p99", 100, 1.5)   # a single volume
    R.assert_equal(one, R.batch_reference(shape, "p99", 100, 1.5)[:1])
    with pytest.raises(IndexError):
        _lib.distribution(hp[2], mk[2])
    with pytest.raises(ValueError):
        _lib.distribution(hp[0], mk[0], bins=0)


def identity_n4(hp, mask):
    return np.asarray(hp, dtype=np.float32).copy()


@pytest.mark.parametrize("own_n4", [False, True], ids=["n4", "identity"])
def test_class_ventilation_distribution(own_n4):
    """After calculate_VDP and again after select_defect("kmeans"): the counts are those of the object's
    own N4HPvent, mask, defectArray and defectArrayLB."""
    from vent_analysis_amd import Vent_Analysis
    shape = (41, 37, 9)
    hp, mk, _, _ = R.batch_inputs(shape)
    va = Vent_Analysis(xenon_array=hp[0].copy(), mask_array=mk[0].astype(np.float64), vox=VOX)
    if own_n4:
        va.N4_bias_correction = identity_n4
    va.calculate_VDP()
    for step in ("run", "kmeans"):
        if step == "kmeans":
            d0 = va.defectArray.copy()
            va.select_defect("kmeans")
            assert not np.array_equal(d0, va.defectArray)
        meta = copy.deepcopy(va.metadata)
        attrs = set(vars(va))
        for norm, bins, hi in (("p99", 100, 1.5), ("mean", 1024, 1.5)):
            out = va.ventilation_distribution(norm, bins, hi)
            ref = R.reference(va.N4HPvent, va.mask, va.defectArray, va.defectArrayLB, norm, bins, hi)
            for k in ("hist", "outside", "slice_counts"):
                assert out[k].dtype == ref[k].dtype and np.array_equal(out[k], ref[k]), (step, norm, k)
            assert np.array_equal(out["edges"], np.arange(bins + 1) * (hi / bins))
            sl = ref["slice_counts"]
            n = np.float64(sl[:, 0].sum())
            assert out["lb_percent"].dtype == np.float64 and out["lb_percent"].shape == (6,)
            assert np.array_equal(out["lb_percent"], 100 * sl[:, 2:].sum(axis=0) / n)
            assert np.array_equal(out["slice_vdp"], 100 * sl[:, 1] / sl[:, 0])   # (every slice holds mask)
            assert out["vdp_from_slices"] == 100 * np.float64(va.defectArray.sum()) / n
            if step == "run":
                assert out["vdp_from_slices"] == va.metadata["VDP"]
            # VDP_lb = 100 (a + b) / n against 100 a / n + 100 b / n: the counts are equal, the
            # percentages to the last float64 bits
            assert 100 * np.float64(sl[:, 2:4].sum()) / n == va.metadata["VDP_lb"]
            assert abs(out["lb_percent"][0] + out["lb_percent"][1] - va.metadata["VDP_lb"]) <= \
                2 * np.spacing(va.metadata["VDP_lb"])
        out = va.ventilation_distribution()   # the defaults
        assert out["hist"].shape == (100,) and np.array_equal(
            out["hist"], R.histogram(va.N4HPvent, va.mask, "p99", 100, 1.5)[0])
        np.testing.assert_equal(va.metadata, meta)   # no metadata key, no attribute
        assert set(vars(va)) == attrs


def test_slice_vdp_is_nan_where_a_slice_holds_no_mask():
    from vent_analysis_amd import Vent_Analysis
    shape = (41, 37, 9)
    hp, mk, _, _ = R.batch_inputs(shape)
    m = mk[0].astype(np.float64)
    m[:, :, [0, 7]] = 0
    va = Vent_Analysis(xenon_array=hp[0].copy(), mask_array=m, vox=VOX)
    va.N4_bias_correction = identity_n4
    va.calculate_VDP()
    out = va.ventilation_distribution()
    sl = out["slice_counts"]
    assert list(np.flatnonzero(np.isnan(out["slice_vdp"]))) == [0, 7] and not sl[[0, 7]].any()
    on = sl[:, 0] > 0
    assert np.array_equal(out["slice_vdp"][on], 100 * sl[on, 1] / sl[on, 0])
    assert np.array_equal(sl, R.slice_counts(va.mask, va.defectArray, va.defectArrayLB))


def test_kernel_time():
    shape = (33, 20, 5)
    B = plain_run(shape, profile=True)
    B.distribution()
    B.distribution("mean", 10, 2.0)
    B.download_distribution()
    ms, launches, nbytes = B.kernel_time("dist_b")
    B.close()
    assert launches == 2 and ms > 0
    assert nbytes == 7.0 * B.shape[0] * np.prod(shape)   # N4 4, mask, defect and LB 1 byte per voxel
