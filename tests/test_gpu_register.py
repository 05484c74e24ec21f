"""GPU: the proton registered to the xenon image of a resident batch (vh_batch_register / vh_batch_shift
and the layers above them) against the numpy reference (register_ref).  The joint histograms are exact
integers and compare under np.array_equal; the scores are float64 within 1e-10 (at most 1024 terms of
|log| <= 26, a few ulp each)."""
import functools

import numpy as np
import pytest

from vent_analysis_amd import _lib

import mask_edit_ref as M
import register_ref as G

pytestmark = pytest.mark.gpu

VOX = (1.5, 1.5, 10.0)
TOL = 1e-10


def studies(shape):
    return 2 if shape == (128, 128, 24) else 4


def same(a, b):
    """Equal dtype, shape and bits (NaN payloads and -0.0 included)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def resident(shape):
    """One batch per shape with the phantom's xenon and proton uploaded, kept for the parametrised cases."""
    n = studies(shape)
    P, X = G.batch(shape)
    B = _lib.Batch(*shape, n)
    B.upload(X[:n], np.ones((n,) + shape, np.uint8))
    B.upload_proton(P[:n])
    return B


def check_against_reference(shape, search, got, planted=None):
    n = studies(shape)
    best, score, status, hist = got
    rh, rs, rbest, gaps = G.reference(shape, search, n)
    wz, wr, wc = 2 * search[2] + 1, 2 * search[0] + 1, 2 * search[1] + 1
    assert best.dtype == np.int32 and best.shape == (n, 3) and status.dtype == np.int32 and status.tolist() == [0] * n
    assert score.dtype == np.float64 and score.shape == (n, wz, wr, wc)
    assert hist.dtype == np.uint32 and hist.shape == (n, wz, wr, wc, 32, 32)
    hist, score = hist.reshape(n, -1, 32, 32), score.reshape(n, -1)
    for q in range(n):
        for i, s in enumerate(G.shifts(search)):
            assert np.array_equal(hist[q, i], rh[q, i]), (q, s, np.argwhere(hist[q, i] != rh[q, i])[:4])
        assert np.abs(score[q] - rs[q]).max() <= TOL, (q, np.abs(score[q] - rs[q]).max())
        assert max(abs(score[q, i] - _lib.mi(hist[q, i])) for i in range(hist.shape[1])) <= TOL
        assert tuple(best[q]) == _lib.register_pick(score[q], search)
    if planted is not None:
        for q in range(min(n, 3)):
            assert gaps[q] >= 1e-6 and rbest[q] == planted[q]            # the reference first
            assert tuple(best[q]) == planted[q], (q, best[q])
    if n == 4:                                                           # a constant proton
        assert (score[3] == 0.0).all() and tuple(best[3]) == (0, 0, 0)


@pytest.mark.parametrize("shape,search,planted", G.CASES, ids=lambda v: str(v).replace(" ", "") if isinstance(v, tuple) else "")
def test_register_equals_the_reference(shape, search, planted):
    check_against_reference(shape, search, resident(shape).register(search, hist=True), planted)


def test_a_window_of_one_shift():
    shape = (41, 37, 9)
    got = resident(shape).register((0, 0, 0), hist=True)
    check_against_reference(shape, (0, 0, 0), got)
    assert got[0].tolist() == [[0, 0, 0]] * 4 and got[1].shape == (4, 1, 1, 1)


def test_an_unregistrable_study_leaves_its_neighbours_alone():
    shape, search, planted = G.CASES[0]
    P, X = G.batch(shape)
    X = X.copy()
    X[1] = 0.0                                    # an all-zero xenon: its maximum is not > 0
    P = P.copy()
    P[2] = np.where(P[2] > 50, np.nan, -1.0)      # F of the proton is empty
    B = _lib.Batch(*shape, 4)
    B.upload(X, np.ones((4,) + shape, np.uint8))
    B.upload_proton(P)
    best, score, status, hist = B.register(search, hist=True)
    B.close()
    assert status.tolist() == [0, 1, 1, 0]
    assert np.isnan(score[1]).all() and np.isnan(score[2]).all() and best[1:3].tolist() == [[0, 0, 0]] * 2
    assert not hist[1].any() and not hist[2].any()
    rh, rs, rbest, _ = G.reference(shape, search)
    for q in (0, 3):
        assert np.array_equal(hist[q].reshape(-1, 32, 32), rh[q])
        assert np.abs(score[q].reshape(-1) - rs[q]).max() <= TOL and tuple(best[q]) == rbest[q]


SHIFTS = np.array([(0, 0, 0), (4, -4, 2), (-4, 4, -2), (-3, 0, 1)], np.int32)   # zero, the full window, negative, mixed


def test_shift_proton_is_the_numpy_shift_and_aligns_the_pair():
    shape, search, planted = G.CASES[0]
    P, X = G.batch(shape)
    B = _lib.Batch(*shape, 4)
    B.upload(X, np.ones((4,) + shape, np.uint8))
    B.upload_proton(P)
    assert same(B.download_proton(), P)
    used = B.shift_proton(SHIFTS)
    assert used.dtype == np.int32 and np.array_equal(used, SHIFTS)
    want = np.stack([G.shift_image(P[q], SHIFTS[q]) for q in range(4)])
    assert same(B.download_proton(), want)                                # NaN, inf and negative voxels move as bits
    B.shift_proton((41, 0, 0))                                            # a whole dimension: zeros
    assert not B.download_proton().any()
    B.upload_proton(P)
    best = B.register(search)[0]
    assert [tuple(b) for b in best[:3]] == planted
    B.shift_proton(best)
    again, score, _ = B.register(search)
    assert again.tolist() == [[0, 0, 0]] * 4
    assert same(B.download_hp(), X)
    B.close()


def test_shift_mask_puts_the_batch_back_to_uploaded_and_the_next_run_sees_the_mask():
    shape = (41, 37, 9)
    P, X = G.batch(shape)
    masks = M.batch_masks(shape)
    hp = np.abs(np.nan_to_num(X, nan=1.0, posinf=2.0, neginf=3.0)) + np.float32(5)
    from vent_analysis_amd.sphere import compact_table_for
    defect = (np.random.default_rng(7).random((4,) + shape) < 0.2).astype(np.uint8)
    table = compact_table_for(VOX, 12, shape)
    B = _lib.Batch(*shape, 4)
    B.upload(hp, masks)
    B.upload_defect(defect)
    B.ci(VOX, table=table)
    ci_before = B.download_ci()
    B.upload_proton(P)
    B.run(B.options(do_n4=False, vox=VOX))
    before = B.download()
    # register reads only: the run's results, the mask, the HPvent and the proton are as they were
    B.register((2, 2, 1), hist=True)
    after = B.download()
    for a, b in zip(before[:4], after[:4]):
        assert (a is None and b is None) or same(a, b)
    assert [r.n_mask for r in before[4]] == [r.n_mask for r in after[4]]
    assert same(B.download_mask(), masks) and same(B.download_hp(), hp) and same(B.download_proton(), P)
    B.shift_proton(SHIFTS)                                                # the proton shift invalidates nothing
    B.download()
    B.upload_defect(defect)
    B.shift_mask(SHIFTS)
    for call in (B.download, lambda: B.select_defect("mean"), B.distribution, B.overlay, B.montage_layout,
                 B.km_cuts):
        with pytest.raises(ValueError):
            call()
    want = np.stack([G.shift_image(masks[q], SHIFTS[q]) for q in range(4)])
    assert want.dtype == np.uint8 and set(np.unique(want[1])) == {0, 2, 255}   # bytes move as they are
    assert same(B.download_mask(), want)
    assert same(B.download_hp(), hp)                                      # HPvent survives
    B.ci(VOX, table=table)                                                # ... and a set_defect map
    for a, b in zip(ci_before, B.download_ci()):
        assert np.array_equal(a, b, equal_nan=True)
    B.run(B.options(do_n4=False, vox=VOX))
    res = B.download()[4]
    got, cnt = B.download_mask(count=True)
    B.close()
    assert same(got, want)
    assert [r.n_mask for r in res] == cnt.tolist() == (want != 0).reshape(4, -1).sum(axis=1).tolist()


def test_host_buffer_form_and_class_method():
    from vent_analysis_amd import Vent_Analysis
    shape, search, planted = G.CASES[3]
    P, X = G.batch(shape)
    rh, rs, rbest, _ = G.reference(shape, search)
    best, score, status, shifted = _lib.register(P, X, search, apply=True)
    assert [tuple(b) for b in best] == rbest and status.tolist() == [0] * 4
    assert np.abs(score.reshape(4, -1) - rs).max() <= TOL
    assert same(shifted, np.stack([G.shift_image(P[q], rbest[q]) for q in range(4)]))
    b1, s1, st1 = _lib.register(P[0].astype(np.float64), X[0], search)      # one 3-D volume, no apply
    assert tuple(b1[0]) == planted[0] and same(s1[0], score[0]) and st1.tolist() == [0]
    va = Vent_Analysis(pickle_dict=dict(HPvent=X[0].copy(), mask=np.ones(shape), vox=list(VOX)))
    keys = set(vars(va))
    va.proton = P[0].astype(np.float64)
    shift, value = va.register_proton(search, apply=False)
    assert shift == planted[0] and value == score[0].max() and same(va.proton, P[0].astype(np.float64))
    shift, value = va.register_proton(search)
    assert shift == planted[0] and va.proton.dtype == np.float64
    assert same(va.proton, G.shift_image(P[0].astype(np.float64), planted[0]))
    assert va.register_proton(search)[0] == (0, 0, 0)                       # it lies on the xenon's voxels now
    assert set(vars(va)) - keys <= {"proton"}                               # no attribute for pickleMe to write


def test_library_argument_errors():
    """The library's own checks (the binding's are bypassed): VH_ERR_ARG, nothing enqueued or changed."""
    shape = (41, 37, 9)
    P, X = G.batch(shape)
    masks = M.batch_masks(shape)
    p = _lib._ptr
    B = _lib.Batch(*shape, 4)
    B.upload(X, masks)
    ok = np.array([2, 2, 1], np.int32)
    score, best = np.zeros((4, 75)), np.zeros((4, 3), np.int32)
    hist = np.zeros((4, 75, 32, 32), np.uint32)
    zero = np.zeros((4, 3), np.int32)
    ERR = _lib.VH_ERR_ARG
    assert B.L.vh_batch_register(B.h, p(ok), p(score), p(best), None, None) == ERR              # no proton
    assert B.L.vh_batch_shift(B.h, _lib.VH_SHIFT_PROTON, p(zero)) == ERR
    assert B.L.vh_batch_download_proton(B.h, p(np.zeros((4,) + shape, np.float32))) == ERR
    with pytest.raises(ValueError):
        B.register()
    B.upload_proton(P)
    assert B.L.vh_batch_download_register_hist(B.h, p(hist)) == ERR                            # before any register
    assert B.L.vh_batch_register(B.h, None, p(score), p(best), None, None) == ERR
    assert B.L.vh_batch_register(B.h, p(ok), None, p(best), None, None) == ERR
    assert B.L.vh_batch_register(B.h, p(ok), p(score), None, None, None) == ERR
    for bad in ((9, 0, 0), (0, 9, 0), (0, 0, 3), (-1, 0, 0), (0, 0, -1)):
        assert B.L.vh_batch_register(B.h, p(np.array(bad, np.int32)), p(score), p(best), None, None) == ERR, bad
        with pytest.raises(ValueError):
            B.register(bad)
    assert B.L.vh_batch_download_register_hist(B.h, p(hist)) == ERR
    for what, s in ((2, zero), (-1, zero), (_lib.VH_SHIFT_PROTON, None), (_lib.VH_SHIFT_MASK, None),
                    (_lib.VH_SHIFT_PROTON, np.array([[0, 0, 0]] * 3 + [[42, 0, 0]], np.int32)),
                    (_lib.VH_SHIFT_MASK, np.array([[0, -38, 0]] + [[0, 0, 0]] * 3, np.int32)),
                    (_lib.VH_SHIFT_MASK, np.array([[0, 0, 0]] * 2 + [[0, 0, 10]] + [[0, 0, 0]], np.int32))):
        assert B.L.vh_batch_shift(B.h, what, p(s)) == ERR, (what, s)
    with pytest.raises(ValueError):
        B.shift_mask((0, 0, 10))
    assert B.L.vh_batch_download_proton(B.h, None) == ERR
    assert same(B.download_proton(), P) and same(B.download_mask(), masks) and same(B.download_hp(), X)
    bs, st = np.zeros(4), np.zeros(4, np.int32)
    assert B.L.vh_batch_register(B.h, p(ok), p(score), p(best), p(bs), p(st)) == _lib.VH_OK     # the nullable pair
    assert B.L.vh_batch_download_register_hist(B.h, p(hist)) == _lib.VH_OK
    assert np.array_equal(bs, score.max(axis=1)) and st.tolist() == [0] * 4
    assert np.array_equal(hist, G.reference(shape, (2, 2, 1))[0])
    B.close()
    # a window that reaches a dimension: the library refuses it, and so does the binding
    small = (4, 8, 2)
    W = _lib.Batch(*small, 1)
    x = np.ones((1,) + small, np.float32)
    W.upload(x, np.ones((1,) + small, np.uint8))
    W.upload_proton(x)
    sc = np.zeros(9 * 17 * 5)
    for bad in ((4, 0, 0), (0, 8, 0), (0, 0, 2)):
        assert W.L.vh_batch_register(W.h, p(np.array(bad, np.int32)), p(sc), p(best), None, None) == ERR, bad
        with pytest.raises(ValueError):
            W.register(bad)
    c = W.ctx
    one = np.array([1, 1, 0], np.int32)
    assert c.L.vh_register(c.h, None, p(x), 4, 8, 2, 1, p(one), p(sc), p(best), None, None) == ERR
    assert c.L.vh_register(c.h, p(x), p(x), 4, 8, 2, 1, None, p(sc), p(best), None, None) == ERR
    assert c.L.vh_register(c.h, p(x), p(x), 4, 8, 2, 1, p(np.array([4, 0, 0], np.int32)), p(sc), p(best), None, None) == ERR
    assert W.register((3, 7, 1))[0].tolist() == [[0, 0, 0]]                # the largest window this shape takes
    W.close()
