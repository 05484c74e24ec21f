"""GPU: the defect table of a resident batch (vh_batch_defect_table and the layers above it) against
the numpy reference (defect_table_ref on top of components_ref).  Every entry is an integer with one
value, so every comparison is exact, over every row of every study: the empty and the full study, the
checkerboard (every key ties in size: the selection), random fills, parts that join only through
another slice.  The kernels have one form; the shapes cover max_rows above V, chunks that end inside the
volume, several chunks, and more components than rows by a factor of 80."""
import functools

import numpy as np
import pytest

from vent_analysis_amd import _lib

import components_ref as K
import defect_table_ref as T
import distribution_ref as DR

pytestmark = pytest.mark.gpu

VOX = (1.5, 1.5, 10.0)
N = K.N_STUDIES
SHAPES = [(2, 2, 1), (5, 3, 1), (41, 37, 9), (64, 64, 24), (8, 8, 70), (300, 280, 2)]
MAX_ROWS = (1, 5, 64, 1024)
PER_STUDY = (1, 2, 1, 7, 40, 2, 3, 2)


def assert_equal(got, ref, what=""):
    """got: a download_defect_table dict; ref: defect_table_ref.cut_batch's."""
    for k in ("stats", "truncated", "rows"):
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (what, k, got[k].dtype, got[k].shape)
    assert np.array_equal(got["stats"], ref["stats"]), (what, got["stats"], ref["stats"])
    assert np.array_equal(got["truncated"], ref["truncated"]), what
    for q in range(got["rows"].shape[0]):
        bad = np.argwhere(got["rows"][q] != ref["rows"][q])
        assert bad.size == 0, (what, q, len(bad), bad[:4].tolist(), got["rows"][q][bad[0][0]].tolist(),
                               ref["rows"][q][bad[0][0]].tolist())


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


@functools.lru_cache(maxsize=None)
def tables(shape, conn):
    return T.batch_tables(K.batch_inputs(shape), conn)


def min_sizes(fulls):
    """The scalar and per-study min_size values of the cases; the last is one above the largest
    component of every study: zero rows."""
    above = tuple(int(f[0, T.SIZE]) + 1 if len(f) else 1 for f in fulls)
    return (1, 2, 40, PER_STUDY, above)


@pytest.mark.parametrize("conn", K.CONNS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_table_equals_the_reference(shape, conn):
    """Every row and the stats, for every max_rows and min_size; source defect (uploaded, no run), no
    signal.  (2, 2, 1): max_rows above V.  (300, 280, 2): the checkerboard has 84 000 components of one
    voxel at 4 neighbours and 42 000 of two at 6, whose rows are its first max_rows roots by index."""
    B = resident(shape)
    fulls = tables(shape, conn)
    B.components("defect", conn)
    truncated = {True: 0, False: 0}
    for ms in min_sizes(fulls):
        for n in MAX_ROWS:
            ref = T.cut_batch(fulls, ms, n)
            B.defect_table(ms, n)
            got = B.download_defect_table()
            assert_equal(got, ref, (ms, n))
            assert not got["rows"][:, :, T.N_SIG:].any()             # norm=None
            for v in ref["truncated"]:
                truncated[bool(v)] += 1
    assert not ref["stats"].any() and (ref["rows"][:, :, 0] == -1).all()   # the last min_size: zero rows everywhere
    assert truncated[False] > 0
    if shape != (2, 2, 1):
        assert truncated[True] > 0
    if shape == (300, 280, 2) and conn in (4, 6):   # every key ties in size: the smallest roots win
        on = np.flatnonzero(K.batch_inputs(shape)[K.CHECKER].ravel())
        ck = T.cut_batch(fulls, 1, 1024)
        if conn == 4:
            assert ck["stats"][K.CHECKER].tolist() == [1024, 84000, 1024, 84000]
            assert ck["rows"][K.CHECKER][:, 0].tolist() == on[:1024].tolist()
        else:                                       # the two slices join: 42 000 columns of two voxels
            assert ck["stats"][K.CHECKER].tolist() == [1024, 42000, 2048, 84000]
            assert ck["rows"][K.CHECKER][:, 0].tolist() == on[::2][:1024].tolist()


def test_some_case_truncates_and_some_does_not():
    """From the reference alone: the cases above hold both kinds, in one study even."""
    fulls = tables((41, 37, 9), 6)
    ref = T.cut_batch(fulls, 1, 5)
    assert ref["truncated"][K.RAND40] and not ref["truncated"][K.FULL] and not ref["truncated"][K.EMPTY]
    assert T.cut_batch(tables((2, 2, 1), 4), 1, 1024)["truncated"].sum() == 0
    assert T.cut_batch(tables((300, 280, 2), 4), 1, 1024)["truncated"][K.CHECKER]


@pytest.mark.parametrize("conn", (4, 6))
def test_boundary_of_the_cut(conn):
    """max_rows equal to a study's qualifying count and one less: not truncated, then truncated by one."""
    shape = (41, 37, 9)
    B = resident(shape)
    fulls = tables(shape, conn)
    B.components("defect", conn)
    seen = []
    for ms in (1, 2, 3, 5):
        nq = int((fulls[K.RAND40][:, T.SIZE] >= ms).sum())
        for n in sorted({min(max(nq, 1), 1024), min(max(nq - 1, 1), 1024)}):
            ref = T.cut_batch(fulls, ms, n)
            B.defect_table(ms, n)
            assert_equal(B.download_defect_table(), ref, (ms, n))
            seen.append((nq, n, bool(ref["truncated"][K.RAND40])))
    assert any(nq == n and not t for nq, n, t in seen) and any(nq == n + 1 and t for nq, n, t in seen), seen


def test_sums_beyond_32_bits():
    """One study of all ones at (1024, 1024, 9), 6 neighbours, against the closed form: the smallest
    shape of these proportions at which a 32-bit coordinate sum wraps (sum_r = V (R - 1) / 2 > 2^32)."""
    R, C, Z = shape = (1024, 1024, 9)
    V = R * C * Z
    B = _lib.Batch(*shape, 1)
    B.upload_defect(np.ones((1,) + shape, np.uint8))
    B.components("defect", 6)
    B.defect_table(1, 5)
    got = B.download_defect_table()
    B.close()
    want = [0, V, V * (R - 1) // 2, V * (C - 1) // 2, V * (Z - 1) // 2, 0, R - 1, 0, C - 1, 0, Z - 1,
            2 * C * Z, 2 * R * Z, 2 * R * C, 0, 0, 0, 0]
    assert want[2] == 9437184 * 1023 // 2 == 4827119616 > 2 ** 32
    assert got["rows"][0, 0].tolist() == want
    assert (got["rows"][0, 1:, 0] == -1).all() and not got["rows"][0, 1:, 1:].any()
    assert got["stats"].tolist() == [[1, 1, V, V]] and not got["truncated"].any()


@functools.lru_cache(maxsize=None)
def signal_run(shape):
    """A batch after a plain run (N4 = identity, no SNR) with the shared volumes as its defect maps, and
    a few voxels inside their components that must not count -- NaN, inf, negative, 70 d -- and one
    exactly 0 that must; they are off the mask, so the run's divisors do not see them."""
    a = K.batch_inputs(shape)
    hp = field(shape, N)
    mk = np.ones((N,) + shape, np.uint8)
    planted = {}
    for q in (K.FULL, K.RAND60, K.SERPENTINE):
        idx = np.flatnonzero(a[q].ravel())[[0, 3, 7, 11, 19, -1]]
        mk[q].reshape(-1)[idx] = 0
        planted[q] = idx
    B = _lib.Batch(*shape, N)
    B.upload(hp, mk)
    opts = B.options(do_n4=False, do_snr=False, do_kmeans=False, vox=VOX)
    B.run(opts)
    res = B.download()[4]
    d = {"mean": np.array([r.mean_anchor for r in res], np.float32), "p99": np.array([r.p99 for r in res], np.float32)}
    for q, idx in planted.items():
        hp[q].reshape(-1)[idx] = [np.nan, np.inf, -0.25, 70.0 * max(d["mean"][q], d["p99"][q]), 0.0, -np.inf]
    B.upload(hp, mk)
    B.run(opts)                                  # the divisors are the masked voxels': unchanged
    res = B.download()[4]
    assert np.array_equal(d["mean"], np.array([r.mean_anchor for r in res], np.float32))
    assert np.array_equal(d["p99"], np.array([r.p99 for r in res], np.float32))
    B.upload_defect(a)
    hp.setflags(write=False)
    return B, hp, d


@pytest.mark.parametrize("norm", ("mean", "p99"))
@pytest.mark.parametrize("shape", [(41, 37, 9), (64, 64, 24)], ids=str)
def test_signal_columns(shape, norm):
    B, hp, d = signal_run(shape)
    a = K.batch_inputs(shape)
    assert np.isfinite(d[norm]).all() and (d[norm] > 0).all()
    for conn, ms, n in ((6, 1, 64), (4, 2, 1024)):
        B.components("defect", conn)
        B.defect_table(ms, n, norm)
        got = B.download_defect_table()
        ref = T.reference(a, conn, ms, n, hp, d[norm])
        assert_equal(got, ref, (conn, ms, n))
        plain = T.cut_batch(tables(shape, conn), ms, n)              # columns 0..13 do not depend on the signal
        assert np.array_equal(got["rows"][:, :, :T.N_SIG], plain["rows"][:, :, :T.N_SIG])
    full = got["rows"][K.FULL]
    assert full[:, T.SUM_FX].max() > 2 ** 32
    used = got["rows"][:, :, 0] >= 0
    assert (got["rows"][:, :, T.N_SIG][used] <= got["rows"][:, :, T.SIZE][used]).all()
    assert (got["rows"][:, :, T.N_SIG] < got["rows"][:, :, T.SIZE]).any()    # the planted voxels do not count
    assert (got["rows"][:, :, T.MIN_FX][used & (got["rows"][:, :, T.N_SIG] > 0)] >= 0).all()
    assert (got["rows"][K.FULL][:, T.MIN_FX][full[:, 0] >= 0] == 0).any()     # the planted 0 counts, as the smallest


def test_read_only():
    shape = (41, 37, 9)
    a = K.batch_inputs(shape)
    B = _lib.Batch(*shape, N)
    B.upload(field(shape, N), a)
    B.run(B.options(do_n4=False, do_kmeans=False, vox=VOX))
    B.ci(VOX, 8)
    B.components("defect", 6, (2, 5, 10))

    def snapshot():
        n4, d, bo, lb, res = B.download(n4=True)
        cc = B.download_components()
        return ([x.tobytes() for x in (n4, d, bo, lb)] + [bytes(r) for r in res] + [x.tobytes() for x in B.download_defect()]
                + [B.download_mask().tobytes()] + [cc[k].tobytes() for k in ("root", "size", "counts", "stats")]
                + [x.tobytes() for x in B.download_ci()])

    before = snapshot()
    B.defect_table(1, 64, "mean")
    first = B.download_defect_table()
    assert snapshot() == before
    B.defect_table(2, 1, None)
    B.download_defect_table()
    assert snapshot() == before
    B.defect_table(1, 64, "mean")                # and the sweep itself is deterministic
    again = B.download_defect_table()
    assert all(first[k].tobytes() == again[k].tobytes() for k in first)
    d = B.download_defect()[0]
    hp, res = B.download(n4=True)[0], B.download()[4]
    B.close()
    assert first["stats"][:, 0].max() > 1
    assert_equal(first, T.reference(d, 6, 1, 64, hp, [r.mean_anchor for r in res]))


def test_lifecycle():
    shape = (41, 37, 9)
    a = K.batch_inputs(shape)
    B = _lib.Batch(*shape, N)
    B.upload(field(shape, N), a)
    with pytest.raises(ValueError):
        B.download_defect_table()                # before any enqueue
    with pytest.raises(ValueError):
        B.defect_table()                         # no components result resident
    B.components("mask", 8)                      # only an upload, no run: the mask's parts
    with pytest.raises(ValueError):
        B.download_defect_table()
    with pytest.raises(ValueError):
        B.defect_table(norm="mean")              # a norm needs a run
    B.defect_table(2, 5)
    assert_equal(B.download_defect_table(), T.cut_batch(tables(shape, 8), 2, 5), "the mask, no run")
    opts = B.options(do_n4=False, do_kmeans=False, vox=VOX)
    B.run(opts)
    with pytest.raises(ValueError):
        B.download_defect_table()                # the run discarded it, with the labelling
    B.upload_defect(a)
    discards = (lambda: B.components("defect", 6), lambda: B.filter_components("defect", 6, 1, 0),
                lambda: B.run(opts))
    for discard in discards:
        B.components("defect", 6)
        B.defect_table(1, 5)
        B.download_defect_table()
        discard()
        with pytest.raises(ValueError):
            B.download_defect_table()
        if discard is not discards[0]:
            with pytest.raises(ValueError):
                B.defect_table(1, 5)             # the filter and the run leave no labelling either
            B.upload_defect(a)
            B.components("defect", 6)
        B.defect_table(1, 5)                     # a new table makes it valid again
        assert_equal(B.download_defect_table(), T.cut_batch(tables(shape, 6), 1, 5), "again")
    B.components("defect", 26)
    B.defect_table(1, 1024)                      # two enqueues, no download between them: the last one's
    B.defect_table((1, 2, 1, 7, 40, 2, 3, 2), 5)
    got = B.download_defect_table()
    assert got["rows"].shape == (N, 5, 18)
    assert_equal(got, T.cut_batch(tables(shape, 26), (1, 2, 1, 7, 40, 2, 3, 2), 5), "the last call")
    B.upload_defect(np.zeros_like(a))            # a snapshot: a later change of the map does not change it
    B.defect_table(1, 64)
    assert_equal(B.download_defect_table(), T.cut_batch(tables(shape, 26), 1, 64), "as it stood at components()")
    B.components("mask", 4)                      # the mask's parts
    B.defect_table(3, 64)
    assert_equal(B.download_defect_table(), T.cut_batch(tables(shape, 4), 3, 64), "the mask")
    B.close()


def test_library_argument_errors():
    """The library's own checks (the binding's are bypassed): VH_ERR_ARG, nothing enqueued -- the result
    of the valid call before them is what a later download returns."""
    shape = (5, 3, 1)
    a = K.batch_inputs(shape)
    B = _lib.Batch(*shape, N)
    B.upload(None, a)
    u32 = lambda v: np.asarray(v, np.uint32)

    def call(ms, n, norm):
        ms = None if ms is None else u32(ms)
        return B.L.vh_batch_defect_table(B.h, _lib._ptr(ms), n, norm)

    assert call([1] * N, 64, -1) == _lib.VH_ERR_ARG                  # no components result
    B.components("mask", 4)
    assert call([1] * N, 3, -1) == _lib.VH_OK
    B._dt = 3
    for n in (0, 1025, -1, 2 ** 31 - 1):
        assert call([1] * N, n, -1) == _lib.VH_ERR_ARG, n
    assert call(None, 3, -1) == _lib.VH_ERR_ARG
    assert call([1] * (N - 1) + [0], 3, -1) == _lib.VH_ERR_ARG
    for norm in (2, -2, 7):
        assert call([1] * N, 3, norm) == _lib.VH_ERR_ARG, norm
    for norm in (0, 1):
        assert call([1] * N, 3, norm) == _lib.VH_ERR_ARG, norm       # a norm without a run
    with pytest.raises(ValueError):
        B.ctx.check(call([1] * N, 0, -1), "vh_batch_defect_table")
    assert_equal(B.download_defect_table(), T.cut_batch(tables(shape, 4), 1, 3))   # the valid call's result
    assert B.L.vh_batch_download_defect_table(B.h, None, None) == _lib.VH_OK       # both nullable
    assert call([2 ** 32 - 1] * N, 1024, -1) == _lib.VH_OK                         # the ends of the ranges are inside
    B._dt = 1024
    got = B.download_defect_table()
    assert not got["stats"].any() and (got["rows"][:, :, 0] == -1).all() and not got["rows"][:, :, 1:].any()
    B.close()


def identity_n4(hp, mask):
    return np.asarray(hp, dtype=np.float32).copy()


def test_class_method():
    """Vent_Analysis.defect_table equals the reference plus table_metrics, and sets nothing."""
    from vent_analysis_amd import Vent_Analysis
    shape = (66, 66, 4)   # (rows enough for calculate_SNR's noise band)
    mk = np.zeros(shape, np.float64)
    mk[8:30, 10:50] = 1
    mk[36:60, 12:52] = 1
    hp = field(shape, 1)[0] * (0.1 + 0.9 * (mk != 0))
    va = Vent_Analysis(xenon_array=hp, mask_array=mk.copy(), vox=VOX)
    va.N4_bias_correction = identity_n4   # (the class's documented caller-supplied N4)
    va.calculate_VDP()
    before = {k: (v.copy() if isinstance(v, (np.ndarray, dict)) else v) for k, v in vars(va).items()}
    for kw, norm in ((dict(), "mean"), (dict(conn=4, min_size=2, max_rows=3, norm="p99"), "p99"),
                     (dict(conn=26, norm=None), None)):
        out = va.defect_table(**kw)
        assert set(vars(va)) == set(before)
        np.testing.assert_equal(dict(vars(va)), before)
        d = (np.asarray(va.defectArray) != 0).astype(np.uint8)
        m, p99 = DR.anchors(va.N4HPvent, va.mask)
        x = None if norm is None else np.asarray(va.N4HPvent, np.float32)[None]
        ref = T.reference(d[None], kw.get("conn", 6), kw.get("min_size", 1), kw.get("max_rows", 64), x,
                          [m if norm == "mean" else p99])
        st = ref["stats"][0]
        assert (out["n_rows"], out["n_qualifying"], out["voxels_in_rows"], out["voxels_qualifying"]) == tuple(st)
        assert out["truncated"] == bool(ref["truncated"][0]) and out["columns"] == _lib.DT_COLUMNS
        assert out["rows"].dtype == np.int64 and np.array_equal(out["rows"], ref["rows"][0][:st[0]])
        for k, v in _lib.table_metrics(ref["rows"][0][:st[0]], VOX).items():
            assert np.array_equal(out[k], v, equal_nan=True), k
        assert out["n_rows"] > 1 and not np.isnan(out["volume_mL"]).any()
        if norm is not None:
            assert (out["rows"][:, T.N_SIG] > 0).all() and np.isfinite(out["mean"]).all()
        else:
            assert np.isnan(out["mean"]).all()


def test_kernel_time():
    shape = (33, 20, 5)
    a = K.batch_inputs(shape)
    B = _lib.Batch(*shape, N)
    B.upload(field(shape, N), a)
    B.run(B.options(do_n4=False, do_kmeans=False, vox=VOX, profile=True))
    B.components("defect", 6)
    B.defect_table(1, 64)
    B.defect_table(1, 5, "mean")
    B.download_defect_table()
    ms, launches, nbytes = B.kernel_time("dtab_b")
    B.close()
    assert launches == 2 and ms > 0
    assert nbytes == 12.0 * N * np.prod(shape)   # the last launch's: root 4 + size 4 + x 4 bytes per voxel
