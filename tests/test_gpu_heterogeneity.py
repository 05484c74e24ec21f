"""GPU: the local ventilation heterogeneity of a resident batch (vh_batch_heterogeneity /
Batch.heterogeneity and the layers above it) against the numpy reference (heterogeneity_ref).  The map
is specified to the last bit and the summary is integer counts: every comparison is exact, over every
voxel of every study, the empty-mask study included."""
import ctypes as ct
import functools

import numpy as np
import pytest

from vent_analysis_amd import _lib

import heterogeneity_ref as H

pytestmark = pytest.mark.gpu

F32 = np.float32
VOX = (1.5, 1.5, 10.0)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == F32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def assert_equal(got, ref, what=""):
    """got: a download_heterogeneity dict; ref: (maps, hist, stats) of the reference."""
    maps, hist, stats = ref
    if got["map"] is not None:
        for q in range(maps.shape[0]):
            assert same_bits(got["map"][q], maps[q]), (what, q, int((got["map"][q].view(np.uint32)
                                                                      != maps[q].view(np.uint32)).sum()))
    assert got["hist"].dtype == np.uint32 and np.array_equal(got["hist"], hist), what
    assert got["stats"].dtype == np.int64 and np.array_equal(got["stats"], stats), (what, got["stats"], stats)
    assert np.array_equal(got["index"], [H.index(s) for s in stats], equal_nan=True), what


def plain_run(shape, n=3, **kw):
    x, mk = H.batch_inputs(shape)[:n], H.batch_masks(shape)[:n]
    B = _lib.Batch(*shape, n)
    B.upload(x, mk)
    B.run(B.options(do_n4=False, do_kmeans=False, vox=VOX, **kw))
    return B


@functools.lru_cache(maxsize=None)
def resident(shape):
    """The batch of a shape after one plain run (N4 = identity), kept resident for the parametrised
    cases."""
    return plain_run(shape)


@pytest.mark.parametrize("radius,min_count", H.PARAMS)
@pytest.mark.parametrize("shape", H.SHAPES, ids=str)
def test_heterogeneity_equals_the_reference(shape, radius, min_count):
    """The map in float32 bits, the histogram and the stats as integers; then the same counts with
    map=False."""
    B = resident(shape)
    B.heterogeneity(radius, min_count, H.BINS, H.HI)
    got = B.download_heterogeneity()
    ref = H.batch_reference(shape, radius, min_count)
    assert got["map"].shape == (3,) + shape and got["hist"].shape == (3, H.BINS) and got["stats"].shape == (3, 4)
    assert np.array_equal(got["edges"], np.arange(H.BINS + 1) * (H.HI / H.BINS)) and got["edges"].dtype == np.float64
    assert_equal(got, ref)
    assert not got["map"][2].view(np.uint32).any() and not got["hist"][2].any() and not got["stats"][2].any()
    assert np.isnan(got["index"][2])
    counts = B.download_heterogeneity(map=False)
    assert counts["map"] is None
    assert_equal(counts, ref, "map=False")


def test_exclude_defect_follows_the_resident_map():
    shape = (41, 37, 9)
    x, mk = H.batch_inputs(shape), H.batch_masks(shape) != 0
    B = plain_run(shape)
    B.select_defect("lb")
    d = B.download_defect()[0]
    assert (d[:2] != 0).any(axis=(1, 2, 3)).all() and ((d != 0) & mk).any()
    for radius, min_count in ((1, 2), (2, 13)):
        B.heterogeneity(radius, min_count, H.BINS, H.HI, exclude_defect=True)
        assert_equal(B.download_heterogeneity(), H.reference(x, mk & (d == 0), radius, min_count), "excluded")
        B.heterogeneity(radius, min_count, H.BINS, H.HI)
        assert_equal(B.download_heterogeneity(), H.batch_reference(shape, radius, min_count), "plain")
    B.close()


def test_it_reads_the_n4_volume():
    """With do_n4 the chain read N4: so does the heterogeneity."""
    shape = (41, 37, 9)
    x, mk = H.batch_inputs(shape)[:2], H.batch_masks(shape)[:2]
    B = _lib.Batch(*shape, 2)
    B.upload(x, mk)
    B.run(B.options(do_n4=True, do_kmeans=False, vox=VOX))
    n4 = B.download(n4=True)[0]
    assert not same_bits(n4, x)
    B.heterogeneity(2, 13, H.BINS, H.HI)
    got = B.download_heterogeneity()
    B.close()
    assert_equal(got, H.reference(n4, mk != 0, 2, 13))


def test_host_buffer_form():
    shape = (64, 64, 24)
    x, mk = H.batch_inputs(shape), H.batch_masks(shape)
    for radius, min_count in H.PARAMS:
        got = _lib.heterogeneity(x, mk, radius, min_count, H.BINS, H.HI)
        assert_equal(got, H.batch_reference(shape, radius, min_count))
        assert np.array_equal(got["edges"], np.arange(H.BINS + 1) * (H.HI / H.BINS))
    one = _lib.heterogeneity(x[1], mk[1] * 7.0, 1, 2, H.BINS, H.HI)      # one 3-D volume, a float mask
    assert one["map"].shape == (1,) + shape
    assert_equal(one, [a[1:2] for a in H.batch_reference(shape, 1, 2)])
    dflt = _lib.heterogeneity(x[0], mk[0])                              # the defaults: radius 1, a majority of 9
    assert dflt["hist"].shape == (1, 100)
    assert_equal(dflt, H.reference(x[:1], mk[:1] != 0, 1, 5, 100, 1.0))
    with pytest.raises(ValueError):
        _lib.heterogeneity(x[0], mk[0], radius=6)
    with pytest.raises(ValueError):
        _lib.heterogeneity(x[0], mk[1:])


def test_class_ventilation_heterogeneity():
    """The object's N4HPvent, mask and defectArray as they stand; nothing on the object changes."""
    from vent_analysis_amd import Vent_Analysis
    shape = (41, 37, 9)
    x, mk = H.batch_inputs(shape), H.batch_masks(shape)
    va = Vent_Analysis(xenon_array=x[1].copy(), mask_array=mk[1].astype(np.float64), vox=VOX)
    with pytest.raises(ValueError):
        va.ventilation_heterogeneity()                                  # no N4HPvent yet
    va.N4HPvent = x[1].astype(np.float64)
    with pytest.raises(ValueError):
        va.ventilation_heterogeneity(exclude_defect=True)               # no defectArray yet
    defect = ((np.random.default_rng(5).random(shape) < 0.2) & (mk[1] != 0)).astype(np.float64)
    va.defectArray = defect
    before = {k: (v.copy() if isinstance(v, (np.ndarray, dict)) else v) for k, v in vars(va).items()}
    out = va.ventilation_heterogeneity(2, 13, H.BINS, H.HI)
    excl = va.ventilation_heterogeneity(2, 13, H.BINS, H.HI, exclude_defect=True)
    dflt = va.ventilation_heterogeneity()
    assert set(vars(va)) == set(before)
    np.testing.assert_equal(dict(vars(va)), before)
    ref = H.batch_reference(shape, 2, 13)
    assert same_bits(out["map"], ref[0][1]) and np.array_equal(out["hist"], ref[1][1])
    assert np.array_equal(out["stats"], ref[2][1]) and out["index"] == H.index(ref[2][1])
    assert out["edges"].shape == (H.BINS + 1,)
    rex = H.reference(x[1:2], (mk[1:2] != 0) & (defect == 0), 2, 13)
    assert same_bits(excl["map"], rex[0][0]) and np.array_equal(excl["hist"], rex[1][0])
    assert np.array_equal(excl["stats"], rex[2][0]) and not np.array_equal(excl["stats"], out["stats"])
    rd = H.reference(x[1:2], mk[1:2] != 0, 1, 5, 100, 1.0)
    assert same_bits(dflt["map"], rd[0][0]) and np.array_equal(dflt["hist"], rd[1][0])


def test_read_only_and_repeatable():
    shape = (41, 37, 9)
    B = plain_run(shape)
    B.distribution("mean", 64, 1.5)

    def snapshot():
        n4, d, bo, lb, res = B.download(n4=True)
        dd = B.download_defect()
        ds = B.download_distribution()
        return ([a.tobytes() for a in (n4, d, bo, lb)] + [bytes(r) for r in res] + [a.tobytes() for a in dd]
                + [ds[k].tobytes() for k in ("hist", "outside", "slice_counts")])

    before = snapshot()
    B.heterogeneity(5, 2, H.BINS, H.HI)
    first = B.download_heterogeneity()
    assert snapshot() == before
    B.heterogeneity(1, 2, 7, 2.0, exclude_defect=True)                   # other parameters replace the result
    B.heterogeneity(1, 2, H.BINS, H.HI)
    second = B.download_heterogeneity()
    assert snapshot() == before
    B.close()
    assert_equal(first, H.batch_reference(shape, 5, 2))
    assert_equal(second, H.batch_reference(shape, 1, 2))
    assert not np.array_equal(first["stats"], second["stats"])


def test_lifecycle():
    shape = (41, 37, 9)
    x, mk = H.batch_inputs(shape), H.batch_masks(shape)
    B = _lib.Batch(*shape, 3)
    B.upload(x, mk)
    with pytest.raises(ValueError):
        B.download_heterogeneity()               # before any run
    with pytest.raises(ValueError):
        B.heterogeneity()                        # without a run
    opts = B.options(do_n4=False, do_kmeans=False, vox=VOX)
    for forget in (lambda: B.run(opts), lambda: B.denoise(9.5, 2.0, 1, 0), lambda: B.edit_mask("erode", 1)):
        B.run(opts)
        B.heterogeneity(1, 2, H.BINS, H.HI)
        B.download_heterogeneity(map=False)
        forget()
        with pytest.raises(ValueError):
            B.download_heterogeneity()           # the result went with the run
    with pytest.raises(ValueError):
        B.heterogeneity()                        # the edit forgot the run
    B.upload(x, mk)
    B.run(opts)
    B.heterogeneity(1, 2, H.BINS, H.HI)          # the batch still works
    assert_equal(B.download_heterogeneity(), H.batch_reference(shape, 1, 2))
    B.close()


def test_library_argument_errors():
    """The library's own checks (the binding's are bypassed): VH_ERR_ARG, nothing enqueued -- the
    result of the valid call before them is what a later download returns."""
    shape = (5, 7, 3)
    B = plain_run(shape)
    call = lambda k, mc, nb, hi, ex=0: B.L.vh_batch_heterogeneity(B.h, k, mc, nb, ct.c_float(hi), ex)  # noqa: E731
    assert call(2, 13, H.BINS, H.HI) == _lib.VH_OK
    B._het = (H.BINS, H.HI)
    for k, mc, nb, hi in ((0, 2, 64, 0.5), (6, 2, 64, 0.5), (1, 1, 64, 0.5), (1, 10, 64, 0.5), (2, 26, 64, 0.5),
                          (5, 122, 64, 0.5), (1, 2, 0, 0.5), (1, 2, 1025, 0.5), (1, 2, 64, 0.0), (1, 2, 64, -1.0),
                          (1, 2, 64, np.inf), (1, 2, 64, np.nan), (1, 2, 64, 16.5)):
        assert call(k, mc, nb, hi) == _lib.VH_ERR_ARG, (k, mc, nb, hi)
    assert call(1, 2, 64, 0.5, 2) == _lib.VH_ERR_ARG
    with pytest.raises(ValueError):
        B.ctx.check(call(0, 2, 64, 0.5), "vh_batch_heterogeneity")
    assert_equal(B.download_heterogeneity(), H.batch_reference(shape, 2, 13))
    assert call(5, 121, 1024, 16.0) == _lib.VH_OK                        # the ends of the ranges are inside
    assert call(1, 9, 1, 0.5) == _lib.VH_OK
    B._het = (1, 0.5)
    got = B.download_heterogeneity()
    B.close()
    assert_equal(got, H.reference(H.batch_inputs(shape), H.batch_masks(shape) != 0, 1, 9, 1, 0.5))


def test_kernel_time():
    shape = (33, 20, 5)
    x = np.stack([H.D.field(shape, 1)] * 2)
    mk = np.stack([H.D.ellipse(shape, 0.4)] * 2)
    B = _lib.Batch(*shape, 2)
    B.upload(x, mk)
    B.run(B.options(do_n4=False, do_kmeans=False, vox=VOX, profile=True))
    B.heterogeneity(1, 2, 10, 1.0)
    B.heterogeneity(3, 2, 10, 1.0, exclude_defect=True)
    got = B.download_heterogeneity()
    ms, launches, nbytes = B.kernel_time("het_b")
    d = B.download_defect()[0]
    B.close()
    assert launches == 2 and ms > 0
    assert nbytes == 10.0 * 2 * np.prod(shape)   # a launch's: x 4, mask 1, defect 1, the map 4 bytes per voxel
    assert_equal(got, H.reference(x, (mk != 0) & (d == 0), 3, 2, 10, 1.0))
