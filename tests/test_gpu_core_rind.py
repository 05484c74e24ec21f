"""GPU: the core-rind analysis of a resident batch (vh_batch_core_rind / Batch.core_rind and the layers
above it) against the numpy reference (core_rind_ref).  The map is an integer distance and the summary
is integer counts: every comparison is exact, over every voxel of every study -- the full, the empty
and the corner-pixel study included.  The search has two forms, chosen by the row's length and not
by the plane's size: (300, 280, 2), a plane past 160 KiB of uint16, takes the rows-in-LDS form like
(64, 64, 24); core_rind_ref.LONG_ROW takes the other one.  Both run here."""
import ctypes as ct
import functools

import numpy as np
import pytest

from vent_analysis_amd import _lib

import core_rind_ref as K
import mask_edit_ref as ME

pytestmark = pytest.mark.gpu

VOX = (1.5, 1.5, 10.0)
N = K.N_STUDIES


def assert_equal(got, ref, what=""):
    """got: a download_core_rind dict; ref: (maps, counts, stats) of the reference."""
    maps, counts, stats = ref
    if got["d2"] is not None:
        assert got["d2"].dtype == np.uint16 and got["d2"].shape == maps.shape, what
        for q in range(maps.shape[0]):
            assert np.array_equal(got["d2"][q], maps[q]), (what, q, int((got["d2"][q] != maps[q]).sum()))
    assert got["counts"].dtype == np.int64 and got["counts"].shape == counts.shape, (what, got["counts"].shape)
    assert np.array_equal(got["counts"], counts), (what, got["counts"], counts)
    assert got["stats"].dtype == np.int64 and np.array_equal(got["stats"], stats), (what, got["stats"], stats)
    assert np.array_equal(got["band_vdp"], _lib.band_vdp(counts), equal_nan=True), what


def field(shape, n):
    """float32 [n][R][C][Z] in (0.05, 1.05): a seeded signal for the tests that need a run."""
    return (np.random.default_rng(31 + int(np.prod(shape))).random((n,) + tuple(shape)) + 0.05).astype(np.float32)


@functools.lru_cache(maxsize=None)
def resident(shape):
    """The batch of a shape with the shared masks and defect maps resident and no run, kept for the
    parametrised cases."""
    B = _lib.Batch(*shape, N)
    B.upload(None, K.batch_masks(shape))
    B.upload_defect(K.batch_defects(shape))
    return B


@pytest.mark.parametrize("thr", K.THRESHOLDS, ids=lambda t: "thr%d" % len(t))
@pytest.mark.parametrize("shape", K.SHAPES + [K.LONG_ROW], ids=str)
def test_core_rind_equals_the_reference(shape, thr):
    """The map, the counts and the stats as integers; then the same counts with map=False and without
    the defect column."""
    assert _lib.core_rind_form(*shape) == ("global" if shape == K.LONG_ROW else "rows")
    B = resident(shape)
    B.core_rind(thresholds=thr)
    got = B.download_core_rind()
    ref = K.batch_reference(shape, thr)
    assert got["thresholds"].dtype == np.uint16 and got["thresholds"].tolist() == list(thr)
    assert_equal(got, ref)
    assert not got["d2"][2].any() and not got["counts"][2].any() and not got["stats"][2].any()   # the empty mask
    assert np.isnan(got["band_vdp"][2]).all()
    counts = B.download_core_rind(map=False)
    assert counts["d2"] is None
    assert_equal(counts, ref, "map=False")
    B.core_rind(thresholds=thr, with_defect=False)
    assert_equal(B.download_core_rind(), K.batch_reference(shape, thr, False), "with_defect=False")


def test_a_plane_deep_enough_to_saturate():
    """All ones, 520 x 516: D2 = min(r + 1, R - r, c + 1, C - c)^2 (test_core_rind_host checks the
    reference against this form) reaches 258^2 = 66564, so the map saturates at 65535, stats keep the
    true maximum, and the bands are those of the saturated value.  R > 510: the column distances do
    not fit a byte here, as they do at every other test shape."""
    R, C = 520, 516
    rr, cc = np.mgrid[0:R, 0:C]
    d2 = (np.minimum(np.minimum(rr + 1, R - rr), np.minimum(cc + 1, C - cc)).astype(np.int64) ** 2)[None, :, :, None]
    mk = np.ones((1, R, C, 1), np.uint8)
    for thr in ((65535,), (40000, 65534)):
        ref = K.reference(mk, mk, thr, d2)
        got = _lib.core_rind(mk, mk, thresholds=thr)
        assert_equal(got, ref, thr)
        assert got["stats"].tolist() == [[R * C, 66564]] and got["d2"].max() == 65535
        assert got["counts"][0, -1, 0] == (d2 >= 65535).sum() == 60      # the voxels 256 or more pixels deep


def test_edges_are_pixels():
    shape = (41, 37, 9)
    B = resident(shape)
    B.core_rind()                                                    # the default edges: 1.5 and 3.5 pixels
    got = B.download_core_rind(map=False)
    assert got["thresholds"].tolist() == [3, 13]
    assert_equal(got, K.batch_reference(shape, (3, 13)))
    B.core_rind(edges=(1.5, 3.5, 8))
    assert_equal(B.download_core_rind(), K.batch_reference(shape, (3, 13, 64)))


@pytest.mark.parametrize("k", [1, 3, 5])
def test_depth_above_k_is_the_device_erosion(k):
    """{D2 > k^2} = vh_batch_edit_mask's erosion by k, both on the device, on masks kept k + 1 pixels
    off the slice border."""
    shape = (64, 64, 24)
    m = K.border_free(K.batch_masks(shape), k)
    A, E = _lib.Batch(*shape, N), _lib.Batch(*shape, N)
    A.upload(None, m)
    E.upload(None, m)
    A.core_rind(thresholds=(), with_defect=False)
    d2 = A.download_core_rind()["d2"]
    E.edit_mask("erode", k)
    eroded = E.download_mask()
    A.close()
    E.close()
    assert m[0].any() and (eroded[0] != 0).any() and (eroded[3] != 0).any()
    assert np.array_equal(d2 > k * k, eroded != 0)
    assert np.array_equal(eroded != 0, np.stack([ME.erode(s, k) for s in m]))


def test_defect_column_follows_the_resident_map():
    shape = (41, 37, 9)
    mk = K.batch_masks(shape)
    thr = (3, 13, 64)
    B = _lib.Batch(*shape, N)
    B.upload(None, mk)
    with pytest.raises(ValueError):
        B.core_rind(thresholds=thr)                                  # no defect maps resident
    B.core_rind(thresholds=thr, with_defect=False)                   # only upload(None, mask), no run
    assert_equal(B.download_core_rind(), K.batch_reference(shape, thr, False), "no run")
    B.upload(field(shape, N) * (mk != 0), mk)
    B.run(B.options(do_n4=False, do_kmeans=False, vox=VOX))
    B.core_rind(thresholds=thr)
    d_run = B.download_defect()[0]
    after_run = B.download_core_rind()
    assert_equal(after_run, K.reference(mk, d_run, thr, K.batch_d2(shape)), "the run's map")
    B.select_defect("lb")
    assert_equal(B.download_core_rind(), K.reference(mk, d_run, thr, K.batch_d2(shape)), "as it stood at the enqueue")
    d_lb = B.download_defect()[0]
    assert not np.array_equal(d_lb, d_run)
    B.core_rind(thresholds=thr)
    after_lb = B.download_core_rind()
    assert_equal(after_lb, K.reference(mk, d_lb, thr, K.batch_d2(shape)), "select_defect's map")
    assert not np.array_equal(after_lb["counts"][:, :, 1], after_run["counts"][:, :, 1])
    assert np.array_equal(after_lb["counts"][:, :, 0], after_run["counts"][:, :, 0])
    B.upload_defect(K.batch_defects(shape))
    B.core_rind(thresholds=thr)
    assert_equal(B.download_core_rind(), K.batch_reference(shape, thr), "upload_defect's map")
    B.close()


def test_lifecycle():
    shape = (41, 37, 9)
    mk = K.batch_masks(shape)
    x = field(shape, N)
    thr = (3, 13)
    B = _lib.Batch(*shape, N)
    B.upload(x, mk)
    with pytest.raises(ValueError):
        B.download_core_rind()                   # before any enqueue
    opts = B.options(do_n4=False, do_kmeans=False, vox=VOX)
    B.run(opts)
    for forget in (lambda: B.run(opts), lambda: B.edit_mask("erode", 0), lambda: B.denoise(9.5, 2.0, 1, 0)):
        B.core_rind(thresholds=thr)
        B.download_core_rind(map=False)
        forget()
        with pytest.raises(ValueError):
            B.download_core_rind()               # the result went with the run
        B.run(opts)
    B.upload(x, mk)
    radii = (1, 2, 0, 3, 1)
    B.edit_mask("erode", radii)
    B.core_rind(thresholds=thr, with_defect=False)
    edited = ME.batch_edit(mk, "erode", radii)
    assert np.array_equal(B.download_mask(), edited)
    assert_equal(B.download_core_rind(), K.reference(edited, None, thr), "the edited mask")
    B.core_rind(thresholds=(2, 5, 10, 17), with_defect=False)        # other thresholds: the new bands
    got = B.download_core_rind()
    assert got["counts"].shape == (N, 5, 2)
    assert_equal(got, K.reference(edited, None, (2, 5, 10, 17)), "other thresholds")
    B.close()


def test_read_only():
    shape = (41, 37, 9)
    mk = K.batch_masks(shape)
    B = _lib.Batch(*shape, N)
    B.upload(field(shape, N), mk)
    B.run(B.options(do_n4=False, do_kmeans=False, vox=VOX))
    B.distribution("mean", 64, 1.5)

    def snapshot():
        n4, d, bo, lb, res = B.download(n4=True)
        dd = B.download_defect()
        ds = B.download_distribution()
        return ([a.tobytes() for a in (n4, d, bo, lb)] + [bytes(r) for r in res] + [a.tobytes() for a in dd]
                + [B.download_mask().tobytes()] + [ds[k].tobytes() for k in ("hist", "outside", "slice_counts")])

    before = snapshot()
    B.core_rind(thresholds=(3, 13, 64))
    first = B.download_core_rind()
    assert snapshot() == before
    B.core_rind(thresholds=tuple(range(1, 32)), with_defect=False)
    second = B.download_core_rind()
    assert snapshot() == before
    d = B.download_defect()[0]
    B.close()
    assert_equal(first, K.reference(mk, d, (3, 13, 64), K.batch_d2(shape)))
    assert_equal(second, K.batch_reference(shape, tuple(range(1, 32)), False))


def test_library_argument_errors():
    """The library's own checks (the binding's are bypassed): VH_ERR_ARG, nothing enqueued -- the
    result of the valid call before them is what a later download returns."""
    shape = (5, 7, 3)
    B = _lib.Batch(*shape, N)
    B.upload(None, K.batch_masks(shape))

    def call(thr, with_defect=0, n=None):
        t = np.asarray(thr, np.uint16)
        return B.L.vh_batch_core_rind(B.h, _lib._ptr(t), len(thr) if n is None else n, with_defect)

    assert call((2, 5)) == _lib.VH_OK
    B._cr = np.array((2, 5), np.uint16)
    assert call((1, 2), 1) == _lib.VH_ERR_ARG                        # with_defect, no defect maps resident
    B.upload_defect(K.batch_defects(shape))
    for thr in (tuple(range(1, 33)), (0,), (0, 3), (3, 0), (4, 4), (1, 7, 7), (5, 4)):
        assert call(thr) == _lib.VH_ERR_ARG, thr                     # n_thr 32, a zero, equal, decreasing
    assert call((1,), 0, -1) == _lib.VH_ERR_ARG
    assert call((1,), 2) == _lib.VH_ERR_ARG and call((1,), -1) == _lib.VH_ERR_ARG
    assert B.L.vh_batch_core_rind(B.h, None, 1, 0) == _lib.VH_ERR_ARG
    with pytest.raises(ValueError):
        B.ctx.check(call((0,)), "vh_batch_core_rind")
    assert_equal(B.download_core_rind(), K.batch_reference(shape, (2, 5), False))
    assert B.L.vh_batch_core_rind(B.h, None, 0, 1) == _lib.VH_OK     # no thresholds: no pointer is needed
    B._cr = np.zeros(0, np.uint16)
    assert_equal(B.download_core_rind(), K.batch_reference(shape, ()))
    assert call(tuple(range(65505, 65536)), 1) == _lib.VH_OK         # the ends of the ranges are inside
    B._cr = np.arange(65505, 65536).astype(np.uint16)
    got = B.download_core_rind()
    B.close()
    assert_equal(got, K.batch_reference(shape, tuple(range(65505, 65536))))


def test_host_buffer_form():
    shape = (64, 64, 24)
    mk, df = K.batch_masks(shape), K.batch_defects(shape)
    got = _lib.core_rind(mk, df, thresholds=(3, 13, 64))
    assert_equal(got, K.batch_reference(shape, (3, 13, 64)))
    assert_equal(_lib.core_rind(mk, edges=(1.5, 3.5, 8)), K.batch_reference(shape, (3, 13, 64), False), "no defect")
    one = _lib.core_rind(mk[1] * 7.0, df[1].astype(np.float32))      # one 3-D volume, float arrays, the default edges
    assert one["d2"].shape == (1,) + shape and one["thresholds"].tolist() == [3, 13]
    assert_equal(one, [a[1:2] for a in K.batch_reference(shape, (3, 13))])
    with pytest.raises(ValueError):
        _lib.core_rind(mk[0], df[1:3])
    with pytest.raises(ValueError):
        _lib.core_rind(mk[0], edges=(2.0, 1.0))


def identity_n4(hp, mask):
    return np.asarray(hp, dtype=np.float32).copy()


def test_class_core_rind():
    """After calculate_VDP: the object's mask and defectArray as they stand; nothing on the object
    changes."""
    from vent_analysis_amd import Vent_Analysis
    shape = (66, 66, 2)   # (rows enough for calculate_SNR's noise band)
    mk = K.batch_masks(shape)[0]
    hp = field(shape, 1)[0] * (0.1 + 0.9 * (mk != 0))
    va = Vent_Analysis(xenon_array=hp, mask_array=mk.astype(np.float64), vox=VOX)
    va.N4_bias_correction = identity_n4   # (the class's documented caller-supplied N4)
    va.calculate_VDP()
    before = {k: (v.copy() if isinstance(v, (np.ndarray, dict)) else v) for k, v in vars(va).items()}
    out = va.core_rind()
    plain = va.core_rind(edges_mm=(4.5,), with_defect=False)
    assert set(vars(va)) == set(before)
    np.testing.assert_equal(dict(vars(va)), before)
    d = np.asarray(va.defectArray) != 0
    assert d.any()
    ref = K.reference(mk[None], d[None], (4, 16))                    # 3 mm and 6 mm are 2 and 4 pixels
    assert out["thresholds"].tolist() == [4, 16] and np.array_equal(out["edges_mm"], [3.0, 6.0])
    assert np.array_equal(out["d2"], ref[0][0]) and np.array_equal(out["counts"], ref[1][0])
    assert out["counts"][:, 0].sum() == out["n_mask"] == np.count_nonzero(mk)
    assert out["counts"][:, 1].sum() == np.count_nonzero(d & (mk != 0))
    assert np.array_equal(out["band_vdp"], _lib.band_vdp(ref[1][0]), equal_nan=True)
    assert out["depth_max_mm"] == 1.5 * float(np.sqrt(np.float64(ref[2][0, 1])))
    rp = K.reference(mk[None], None, (9,))
    assert plain["thresholds"].tolist() == [9] and np.array_equal(plain["counts"], rp[1][0])
    assert not plain["counts"][:, 1].any() and np.array_equal(plain["d2"], out["d2"])


def test_kernel_time():
    shape = (33, 20, 5)
    mk = K.batch_masks(shape)
    B = _lib.Batch(*shape, N)
    B.upload(field(shape, N), mk)
    B.run(B.options(do_n4=False, do_kmeans=False, vox=VOX, profile=True))
    B.core_rind(thresholds=(2,))
    B.core_rind(thresholds=(3, 13), with_defect=False)
    got = B.download_core_rind()
    ms, launches, nbytes = B.kernel_time("depth_b")
    B.close()
    assert launches == 2 and ms > 0
    assert nbytes == 3.0 * N * np.prod(shape)    # a launch's: mask 1, (no defect,) the map 2 bytes per voxel
    assert_equal(got, K.batch_reference(shape, (3, 13), False))
