"""GPU: the connected components of a resident batch (vh_batch_components / vh_batch_filter_components
and the layers above them) against the scipy reference (components_ref).  Every output is an integer
with one canonical value -- the root is the smallest linear index of the component -- so every
comparison is exact, over every voxel and every count of every study: the empty and the full study, the
checkerboard, random fills around the percolation point, the serpentine through every tile, parts that
join only through another slice and lines that hold by diagonal steps over tile corners.  The kernels
have one form; the shapes cover one tile, partial tiles, several tiles both ways and Z split in three."""
import functools

import numpy as np
import pytest

from vent_analysis_amd import _lib

import components_ref as K

pytestmark = pytest.mark.gpu

VOX = (1.5, 1.5, 10.0)
N = K.N_STUDIES
KEYS = ("root", "size", "counts", "stats")


def assert_equal(got, ref, what=""):
    """got: a download_components dict; ref: components_ref.reference's."""
    for k in KEYS:
        if got[k] is None:
            continue
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (what, k, got[k].dtype, got[k].shape)
        if got[k].ndim == 4:
            for q in range(got[k].shape[0]):
                assert np.array_equal(got[k][q], ref[k][q]), (what, k, q, int((got[k][q] != ref[k][q]).sum()))
        else:
            assert np.array_equal(got[k], ref[k]), (what, k, got[k], ref[k])


def field(shape, n):
    """float32 [n][R][C][Z] in (0.05, 1.05): a seeded signal for the tests that need a run."""
    return (np.random.default_rng(57 + int(np.prod(shape))).random((n,) + tuple(shape)) + 0.05).astype(np.float32)


@functools.lru_cache(maxsize=None)
def resident(shape):
    """The batch of a shape with the shared inputs resident as the mask and as the defect map, no run,
    kept for the parametrised cases (nothing in them changes either)."""
    B = _lib.Batch(*shape, N)
    B.upload(None, K.batch_inputs(shape))
    B.upload_defect(K.batch_inputs(shape))
    return B


def test_a_batch_has_no_volume_of_one_voxel():
    """(1, 1, 1) is no shape of a batch (R, C >= 2, as for every other call): the smallest volume the
    kernels can be given is (2, 2, 1), the first of the shared shapes."""
    with pytest.raises(ValueError):
        _lib.components(np.ones((1, 1, 1), np.uint8))
    assert K.SHAPES[0] == (2, 2, 1)


@pytest.mark.parametrize("conn", K.CONNS)
@pytest.mark.parametrize("shape", K.SHAPES, ids=str)
def test_components_equal_the_reference(shape, conn):
    """Every voxel's root and size and every count, for the three edge sets; the partial downloads; the
    mask as the source."""
    B = resident(shape)
    for edges in K.EDGE_SETS:
        ref = K.batch_reference(shape, conn, edges)
        B.components("defect", conn, edges)
        got = B.download_components()
        assert got["edges"].dtype == np.uint32 and got["edges"].tolist() == list(edges)
        assert_equal(got, ref, edges)
    st = got["stats"]
    assert st[K.EMPTY].tolist() == [0, 0, 0, -1] and st[K.FULL, 0] == np.prod(shape)
    if min(shape[:2]) >= 8:   # the inputs are not trivial: many components, and one that spans several tiles
        assert st[:, 1].max() > 1
        if shape[0] > K.TILE[0]:
            assert K.tiles_spanned(got["root"][K.SERPENTINE], st[K.SERPENTINE, 3]) > 1
    part = B.download_components(root=False)
    assert part["root"] is None and part["size"] is not None
    assert_equal(part, ref, "root=False")
    part = B.download_components(root=False, size=False)
    assert part["root"] is None and part["size"] is None
    assert_equal(part, ref, "counts only")
    B.components("mask", conn, K.EDGE_SETS[1])
    assert_equal(B.download_components(size=False), K.batch_reference(shape, conn, K.EDGE_SETS[1]), "mask")


FILTERS = [   # min_size, keep_largest: scalars or one value per study
    (5, 0), (1, 2), (3, 1), (1, 8),
    ((1, 2, 1, 7, 40, 2, 3, 2), (0, 1, 8, 3, 0, 1, 2, 3)),
]


@pytest.mark.parametrize("conn", K.CONNS)
@pytest.mark.parametrize("shape", [(5, 3, 1), (41, 37, 9), (64, 64, 24), (130, 70, 3), (8, 8, 70)], ids=str)
def test_filter_equals_the_reference(shape, conn):
    """min_size alone, keep_largest alone, both, per-study values, keep_largest above the number of
    components (the checkerboard at 4 neighbours holds ties throughout: the smaller roots stay); the
    kept voxels keep their byte values; a second pass changes nothing; components() after the filter
    reports no component below min_size."""
    a = K.batch_inputs(shape)
    B = _lib.Batch(*shape, N)
    for ms, kl in FILTERS:
        ref, ref_kept = K.filter_reference(a, conn, ms, kl)
        B.upload(None, a)
        kept = B.filter_components("mask", conn, ms, kl)
        out = B.download_mask()
        assert kept.dtype == np.int64 and np.array_equal(kept, ref_kept), (ms, kl, kept, ref_kept)
        for q in range(N):
            assert np.array_equal(out[q], ref[q]), (ms, kl, q, int((out[q] != ref[q]).sum()))
        with pytest.raises(ValueError):
            B.download_components()                      # the filter's labelling is no components() result
        again = B.filter_components("mask", conn, ms, kl)
        assert np.array_equal(again, kept) and np.array_equal(B.download_mask(), out)   # idempotent
        B.components("mask", conn, (2,))
        got = B.download_components()
        assert_equal(got, K.reference(ref, conn, (2,)), "after the filter")
        msv = np.broadcast_to(np.asarray(ms), (N,))
        for q in range(N):
            s = got["size"][q]
            assert not ((s > 0) & (s < msv[q])).any()
            assert got["stats"][q, 1] == kept[q, 0] and got["stats"][q, 0] == kept[q, 1]
    B.close()
    if shape == (41, 37, 9) and conn == 4:
        ck = K.filter_reference(a, 4, 1, 8)
        assert ck[1][K.CHECKER].tolist() == [8, 8]                   # eight of the equal components: the first eight
        assert np.flatnonzero(ck[0][K.CHECKER].ravel()).tolist() == np.flatnonzero(a[K.CHECKER].ravel())[:8].tolist()


def test_filter_of_the_defect_source():
    """After a run: the filtered map is the resident defect map, the border is vh_border of it, the
    mask, the run's results and download_defect's count stay (as after upload_defect), and the mask
    source forgets the run."""
    shape = (41, 37, 9)
    a = K.batch_inputs(shape)
    mk = np.ones((N,) + shape, np.uint8)
    B = _lib.Batch(*shape, N)
    B.upload(field(shape, N), mk)
    B.run(B.options(do_n4=False, do_kmeans=False, vox=VOX))
    run_maps = B.download()
    count_run = B.download_defect()[2]
    B.upload_defect(a)
    B.components("defect", 6, (2, 10))
    before = B.download_components()
    kept = B.filter_components("defect", 6, (1, 2, 1, 7, 40, 2, 3, 2), (0, 1, 8, 3, 0, 1, 2, 3))
    ref, ref_kept = K.filter_reference(a, 6, (1, 2, 1, 7, 40, 2, 3, 2), (0, 1, 8, 3, 0, 1, 2, 3))
    assert np.array_equal(kept, ref_kept)
    d, bo, cnt = B.download_defect()
    assert np.array_equal(d, ref) and (d != a).any()
    assert np.array_equal(bo, _lib.border(ref))
    assert np.array_equal(cnt, count_run)                            # not updated: the filtered count is kept[:, 1]
    assert np.array_equal(B.download_mask(), mk)
    B.ci(VOX, 8)                                                     # the CI of the filtered map, as after upload_defect
    F = _lib.Batch(*shape, N)
    F.upload_defect(ref)
    F.ci(VOX, 8)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(B.download_ci(), F.download_ci()))
    F.close()
    after = B.download()                                             # the run is still there
    assert np.array_equal(after[3], run_maps[3]) and np.array_equal(after[1], ref)
    assert [bytes(r) for r in after[4]] == [bytes(r) for r in run_maps[4]]
    with pytest.raises(ValueError):
        B.download_components()                                      # discarded by the filter
    assert_equal(before, K.batch_reference(shape, 6, (2, 10)), "before the filter")
    B.components("defect", 6)                                        # the filtered map is the source now
    assert_equal(B.download_components(), K.reference(ref, 6, ()), "the filtered map")
    B.filter_components("mask", 6, 1, 1)                             # the mask source forgets the run
    with pytest.raises(ValueError):
        B.download_defect()
    with pytest.raises(ValueError):
        B.download_components()
    B.close()


def test_lifecycle():
    shape = (41, 37, 9)
    a = K.batch_inputs(shape)
    B = _lib.Batch(*shape, N)
    B.upload(field(shape, N), a)
    with pytest.raises(ValueError):
        B.download_components()                  # before any enqueue
    with pytest.raises(ValueError):
        B.components("defect")                   # no defect maps resident
    with pytest.raises(ValueError):
        B.filter_components("defect")
    B.components("mask", 8, (2,))                # only an upload, no run
    assert_equal(B.download_components(), K.batch_reference(shape, 8, (2,)), "no run")
    opts = B.options(do_n4=False, do_kmeans=False, vox=VOX)
    B.run(opts)
    for forget in (lambda: B.run(opts), lambda: B.edit_mask("erode", 0), lambda: B.filter_components("mask", 6, 1, 0)):
        B.components("defect", 6)
        B.download_components(root=False, size=False)
        forget()
        with pytest.raises(ValueError):
            B.download_components()              # the result went with the run
        B.run(opts)
    d_run = B.download_defect()[0]
    B.components("defect", 26, (2, 5))
    B.select_defect("lb")                        # a snapshot: a later change of the map does not change it
    B.upload_defect(a)
    assert_equal(B.download_components(), K.reference(d_run, 26, (2, 5)), "as it stood at the enqueue")
    B.components("defect", 4, ())                # again: the last call's result, with its own classes
    got = B.download_components()
    assert got["counts"].shape == (N, 1, 2)
    assert_equal(got, K.batch_reference(shape, 4, ()), "upload_defect's map")
    B.close()


def test_read_only():
    shape = (41, 37, 9)
    a = K.batch_inputs(shape)
    B = _lib.Batch(*shape, N)
    B.upload(field(shape, N), a)
    B.run(B.options(do_n4=False, do_kmeans=False, vox=VOX))
    B.distribution("mean", 64, 1.5)
    B.core_rind(thresholds=(3, 13))
    B.ci(VOX, 8)                                 # the CI of the run's maps: components leaves it as it is

    def snapshot():
        n4, d, bo, lb, res = B.download(n4=True)
        dd = B.download_defect()
        ds = B.download_distribution()
        cr = B.download_core_rind()
        return ([x.tobytes() for x in (n4, d, bo, lb)] + [bytes(r) for r in res] + [x.tobytes() for x in dd]
                + [B.download_mask().tobytes()] + [ds[k].tobytes() for k in ("hist", "outside", "slice_counts")]
                + [cr[k].tobytes() for k in ("d2", "counts", "stats")] + [x.tobytes() for x in B.download_ci()])

    before = snapshot()
    B.components("defect", 6, (2, 5, 10))
    first = B.download_components()
    assert snapshot() == before
    B.components("mask", 26, tuple(range(2, 33)))
    second = B.download_components()
    assert snapshot() == before
    d = B.download_defect()[0]
    B.close()
    assert_equal(first, K.reference(d, 6, (2, 5, 10)))
    assert_equal(second, K.batch_reference(shape, 26, tuple(range(2, 33))))


def test_library_argument_errors():
    """The library's own checks (the binding's are bypassed): VH_ERR_ARG, nothing enqueued -- the result
    of the valid call before them is what a later download returns, and the source is untouched."""
    shape = (5, 3, 1)
    a = K.batch_inputs(shape)
    B = _lib.Batch(*shape, N)
    B.upload(None, a)
    u32 = lambda v: np.asarray(v, np.uint32)
    i32 = lambda v: np.asarray(v, np.int32)

    def comp(source, conn, edges, n=None):
        e = u32(edges)
        return B.L.vh_batch_components(B.h, source, conn, _lib._ptr(e), len(edges) if n is None else n)

    def filt(source, conn, ms, kl):
        ms = None if ms is None else u32(ms)
        kl = None if kl is None else i32(kl)
        return B.L.vh_batch_filter_components(B.h, source, conn, _lib._ptr(ms), _lib._ptr(kl), None)

    assert comp(1, 4, (2, 3)) == _lib.VH_OK
    B._cc = u32((2, 3))
    assert comp(0, 6, ()) == _lib.VH_ERR_ARG                         # VH_CC_DEFECT, no defect maps resident
    assert filt(0, 6, [1] * N, None) == _lib.VH_ERR_ARG
    B.upload_defect(a)
    for source in (-1, 2):
        assert comp(source, 6, ()) == _lib.VH_ERR_ARG and filt(source, 6, [1] * N, None) == _lib.VH_ERR_ARG
    for conn in (0, 5, 7, 18, 27, -6):
        assert comp(0, conn, ()) == _lib.VH_ERR_ARG and filt(0, conn, [1] * N, None) == _lib.VH_ERR_ARG
    for edges in ((1,), (0, 2), (2, 2), (3, 2), (2, 5, 5), tuple(range(2, 34))):
        assert comp(0, 6, edges) == _lib.VH_ERR_ARG, edges
    assert comp(0, 6, (2,), -1) == _lib.VH_ERR_ARG
    assert B.L.vh_batch_components(B.h, 0, 6, None, 1) == _lib.VH_ERR_ARG
    assert filt(0, 6, None, None) == _lib.VH_ERR_ARG
    assert filt(0, 6, [1] * (N - 1) + [0], None) == _lib.VH_ERR_ARG
    assert filt(0, 6, [1] * N, [0] * (N - 1) + [9]) == _lib.VH_ERR_ARG
    assert filt(0, 6, [1] * N, [-1] + [0] * (N - 1)) == _lib.VH_ERR_ARG
    with pytest.raises(ValueError):
        B.ctx.check(comp(0, 3, ()), "vh_batch_components")
    assert_equal(B.download_components(), K.batch_reference(shape, 4, (2, 3)))   # the valid call's result
    assert np.array_equal(B.download_mask(), a)
    assert B.L.vh_batch_components(B.h, 0, 26, None, 0) == _lib.VH_OK   # no edges: no pointer is needed
    B._cc = u32(())
    assert_equal(B.download_components(), K.batch_reference(shape, 26, ()))
    assert filt(1, 8, [2 ** 32 - 1] * N, [8] * N) == _lib.VH_OK         # the ends of the ranges are inside
    assert not B.download_mask().any()
    B.close()


def test_host_buffer_forms():
    shape = (64, 64, 24)
    a = K.batch_inputs(shape)
    got = _lib.components(a, conn=26, edges=(2, 5, 10, 100, 1000))
    assert_equal(got, K.batch_reference(shape, 26, (2, 5, 10, 100, 1000)))
    one = _lib.components(a[K.RAND40].astype(np.float32))            # one 3-D volume, a float array, the defaults
    assert one["root"].shape == (1,) + shape and one["edges"].shape == (0,)
    assert_equal(one, {k: v[K.RAND40:K.RAND40 + 1] for k, v in K.batch_reference(shape, 6, ()).items()})
    out, kept = _lib.filter_components(a, conn=6, min_size=4, keep_largest=(0, 1, 2, 3, 4, 5, 6, 7))
    ref, ref_kept = K.filter_reference(a, 6, 4, (0, 1, 2, 3, 4, 5, 6, 7))
    assert out.dtype == np.uint8 and np.array_equal(out, ref) and np.array_equal(kept, ref_kept)
    assert set(np.unique(out[K.RAND60])) == {0, 1, 2, 255}            # the byte values stay
    # three parts of 64 voxels at 4 neighbours: the two with the smaller roots stay, row 0 of slice 0
    # (root 0) and column 0 of slice 1 (root 1); the last row goes
    two, kept = _lib.filter_components(a[K.BRIDGE] != 0, conn=4, keep_largest=2)
    assert kept.tolist() == [[2, 128]] and two[0, 0, :, 0].all() and two[0, :, 0, 1].all() and two.sum() == 128


def identity_n4(hp, mask):
    return np.asarray(hp, dtype=np.float32).copy()


def test_class_methods():
    """defect_components sets nothing; filter_defects updates defectArray and defectBorder; clean_mask
    keeps the two largest parts of the mask."""
    from vent_analysis_amd import Vent_Analysis
    shape = (66, 66, 4)   # (rows enough for calculate_SNR's noise band)
    mk = np.zeros(shape, np.float64)
    mk[8:30, 10:50] = 1
    mk[36:60, 12:52] = 1
    mk[2:4, 30:33, 1] = 1                                            # a speck: a third part
    hp = field(shape, 1)[0] * (0.1 + 0.9 * (mk != 0))
    va = Vent_Analysis(xenon_array=hp, mask_array=mk.copy(), vox=VOX)
    va.N4_bias_correction = identity_n4   # (the class's documented caller-supplied N4)
    va.calculate_VDP()
    before = {k: (v.copy() if isinstance(v, (np.ndarray, dict)) else v) for k, v in vars(va).items()}
    out = va.defect_components(conn=6, edges=(2, 10))
    assert set(vars(va)) == set(before)
    np.testing.assert_equal(dict(vars(va)), before)
    d = np.asarray(va.defectArray)
    ref = K.reference((d != 0)[None], 6, (2, 10))
    assert np.array_equal(out["root"], ref["root"][0]) and np.array_equal(out["size"], ref["size"][0])
    assert np.array_equal(out["counts"], ref["counts"][0]) and out["n_components"] == ref["stats"][0, 1] > 1
    ml = 0.15 * 0.15 * 1.0
    assert out["voxel_mL"] == float(np.prod(np.divide(VOX, 10))) and abs(out["voxel_mL"] - ml) < 1e-12
    assert out["largest_mL"] == out["largest"] * out["voxel_mL"]
    assert np.array_equal(out["class_mL"], ref["counts"][0][:, 1] * out["voxel_mL"])
    assert out["n_defect_voxels"] == np.count_nonzero(d)
    fr, fk = K.filter_reference((d != 0)[None].astype(np.uint8), 6, 3, 0)
    nc, nv = va.filter_defects(3, conn=6)
    assert (nc, nv) == tuple(fk[0]) and 0 < nv < np.count_nonzero(d)
    assert np.array_equal(va.defectArray, d * (fr[0] != 0)) and va.defectArray.dtype == d.dtype
    assert np.array_equal(va.defectBorder, _lib.border(fr)[0] == 1)
    new = va.clean_mask()                                            # keep_largest = 2: the speck goes
    want = mk.copy()
    want[2:4, 30:33, 1] = 0
    assert new is va.mask and np.array_equal(new, want) and new.dtype == mk.dtype
    assert np.array_equal(va.mask_border, va.calculateBorder(want))
    assert va.metadata['LungVolume'] == np.sum(want == 1) * np.prod(np.divide(VOX, 10)) / 1000


def test_kernel_time():
    shape = (33, 20, 5)
    a = K.batch_inputs(shape)
    B = _lib.Batch(*shape, N)
    B.upload(field(shape, N), a)
    B.run(B.options(do_n4=False, do_kmeans=False, vox=VOX, profile=True))
    B.components("defect", 6)
    B.components("mask", 26, (2, 5))
    got = B.download_components()
    ms, launches, nbytes = B.kernel_time("comp_b")
    B.close()
    assert launches == 2 and ms > 0
    assert nbytes == 9.0 * N * np.prod(shape)    # a launch's: the source 1, the root 4, the size 4 bytes per voxel
    assert_equal(got, K.batch_reference(shape, 26, (2, 5)))
