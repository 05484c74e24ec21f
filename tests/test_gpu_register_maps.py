"""GPU: the fine registration of a resident batch (vh_batch_register_maps and the layers above it) against
the numpy reference (register_maps_ref).  Histograms compare exactly; scores within 1e-10 of the reference
and of vh_mi on the device's own histogram (at most 1024 terms of a double sum, as test_gpu_register)."""
import numpy as np
import pytest

from vent_analysis_amd import _lib

import register_maps_ref as M
import register_ref as G
import resample_ref as S

pytestmark = pytest.mark.gpu

VOX = (1.5, 1.5, 10.0)
TOL = 1e-10


def same(a, b):
    """Equal dtype, shape and bits."""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def resident(src, X, profile=False):
    n, shape = len(X), X.shape[1:]
    B = _lib.Batch(*shape, n)
    B.upload(X, np.ones((n,) + shape, np.uint8))
    if profile:
        B.run(B.options(do_n4=False, do_kmeans=False, vox=VOX, profile=True))   # (turns the kernel timers on)
    B.upload_proton_src(src)
    return B


def check(got, want, lists, home=None):
    """One register_maps(..., hist=True) result against (hist, score, best, status) of the reference."""
    best, best_map, score, status, hist = got
    rh, rs, rbest, rstatus = want
    n = len(rh)
    count = [len(l) for l in lists[0]]
    Kr, Kc, Kz = count
    assert best.dtype == np.int32 and best.shape == (n, 3) and status.dtype == np.int32
    assert status.tolist() == rstatus.tolist()
    assert score.dtype == np.float64 and score.shape == (n, Kz, Kr, Kc)
    assert hist.dtype == np.uint32 and hist.shape == (n, Kz, Kr, Kc, 32, 32)
    assert best_map.dtype == np.float64 and best_map.shape == (n, 3, 2)
    h, s = hist.reshape(n, -1, 32, 32), score.reshape(n, -1)
    for q in range(n):
        for i, k in enumerate(M.candidates(count)):
            assert np.array_equal(h[q, i], rh[q, i]), (q, k, np.argwhere(h[q, i] != rh[q, i])[:4].tolist())
        if rstatus[q]:
            assert np.isnan(s[q]).all()
        else:
            assert np.abs(s[q] - rs[q]).max() <= TOL, (q, np.abs(s[q] - rs[q]).max())
            assert max(abs(s[q, i] - _lib.mi(h[q, i])) for i in range(h.shape[1])) <= TOL
        assert tuple(best[q]) == _lib.register_maps_pick(score[q], home)
        if rstatus[q] or M.gap(rs[q]) > 2 * TOL:                    # (closer scores may order either way within TOL)
            assert tuple(best[q]) == rbest[q], (q, best[q], rbest[q])
        picked = [lists[q][a][best[q][a]] for a in range(3)]
        assert same(best_map[q], np.asarray(picked, np.float64)), (q, best_map[q], picked)


def run_case(case, profile=False):
    src, X, lists = M.batch(case)
    B = resident(src, X, profile)
    got = B.register_maps(M.axis_maps(lists), hist=True)
    check(got, M.reference(case), lists)
    return B, got


@pytest.mark.parametrize("case", [1, 2, 3, 5, 6])
def test_register_maps_equals_the_reference(case):
    B, got = run_case(case)
    B.close()
    src_shape, dst_shape, n, planted = M.CASES[case]
    count = [len(l) for l in M.batch(case)[2][0]]
    assert count == {1: [9, 9, 3], 2: [9, 9, 1], 3: [3, 17, 5], 5: [1, 1, 1], 6: [3, 3, 1]}[case]
    if planted:                                                     # the reference first, then the device
        _, rs, rbest, _ = M.reference(case)
        for q, k in enumerate(planted):
            assert rbest[q] == k and M.gap(rs[q]) >= M.MIN_GAP
            assert tuple(got[0][q]) == k, (q, got[0][q], k)
    if case == 3:                                                   # the skip rule and dropped taps were exercised
        lists = M.batch(3)[2][0]
        assert int(S.taps(40, 37, 0.6, 25.0)[1].min()) == 0 and int(S.taps(64, 41, 1.7, -7.25)[1].min()) == 0
        assert int(S.taps(12, 9, 1.3, 0.2)[1].max()) > 2
        tot = M.reference(3)[0][0].sum(axis=(1, 2))
        assert tot.min() < tot.max() <= 41 * 37 * 9


def test_eight_row_taps_and_the_chunked_r_list(monkeypatch):
    """Row scales 3.9 and 4.0: eight taps.  Under the default budget a band serves both r candidates from
    one slab; under a small one the slab holds one row's taps under one candidate, so the r list is chunked;
    under a middling one the band is short.  The same counts every time."""
    assert int(S.taps(160, 41, 3.9, 0.0)[1].max()) == 8
    for kb in (None, "16", "24", "40"):
        if kb is None:
            monkeypatch.delenv("VH_RM_LDS_KB", raising=False)
        else:
            monkeypatch.setenv("VH_RM_LDS_KB", kb)
        B, _ = run_case(4)
        B.close()


def test_the_bench_shape_takes_the_fused_kernel():
    B, got = run_case(7, profile=True)
    ms, launches, _ = B.kernel_time("register_maps_b")
    B.close()
    assert launches == 1 and ms > 0
    assert got[2].shape == (2, 1, 3, 3)


def test_the_integer_window_is_a_special_case():
    """Source = the proton itself, scale 1, integer offsets: the histograms of Batch.register."""
    shape, search = (41, 37, 9), (4, 4, 2)
    P, X = G.batch(shape)
    B = resident(P, X)
    B.upload_proton(P)
    wbest, wscore, wstatus, whist = B.register(search, hist=True)
    lists = [np.asarray([(1.0, float(d)) for d in range(-s, s + 1)]) for s in search]
    best, best_map, score, status, hist = B.register_maps(lists, hist=True)
    B.close()
    assert np.array_equal(hist, whist) and hist.sum() > 0           # (the two indices run in the same order)
    assert np.abs(score - wscore).max() <= TOL and status.tolist() == wstatus.tolist()
    assert (best - np.asarray(search)).tolist() == wbest.tolist()
    assert best_map[:, :, 0].tolist() == [[1.0] * 3] * 4 and best_map[:, :, 1].tolist() == wbest.astype(float).tolist()


def test_two_calls_with_different_counts():
    """Buffers grow and the histograms are zeroed again: a small search, a large one, the small one again."""
    src, X, lists = M.batch(1)
    small = [[l[0][3:6], l[1][4:5], l[2][1:3]] for l in lists]
    want_small = M.reference_of(src, X, small)
    B = resident(src, X)
    check(B.register_maps(M.axis_maps(small), hist=True), want_small, small)
    check(B.register_maps(M.axis_maps(lists), hist=True), M.reference(1), lists)
    check(B.register_maps(M.axis_maps(small), hist=True), want_small, small)
    # home: ties aside it changes nothing but the unregistrable pick
    got = B.register_maps(M.axis_maps(small), home=(2, 0, 1), hist=True)
    check(got, M.reference_of(src, X, small, (2, 0, 1)), small, (2, 0, 1))
    B.close()


def test_an_unregistrable_study_leaves_its_neighbours_alone():
    src, X, lists = M.batch(1)
    src, X = src.copy(), X.copy()
    src[1] = 0.0                                                    # an all-zero source: its maximum is not > 0
    X[2] = np.where(X[2] > 20, np.nan, -1.0)                        # F of the xenon is empty
    want = M.reference_of(src, X, lists)
    assert want[3].tolist() == [0, 1, 1, 0] and want[2][1] == (4, 4, 1)
    B = resident(src, X)
    got = B.register_maps(M.axis_maps(lists), hist=True)
    check(got, want, lists)
    assert not got[4][1].any() and not got[4][2].any() and got[0][1:3].tolist() == [[4, 4, 1]] * 2
    ref = M.reference(1)
    for q in (0, 3):                                                # ... as if the others were not there
        assert np.array_equal(got[4][q].reshape(-1, 32, 32), ref[0][q])
    got = B.register_maps(M.axis_maps(lists), home=(0, 8, 2))
    assert got[0][1:3].tolist() == [[0, 8, 2]] * 2 and got[3].tolist() == [0, 1, 1, 0]
    B.close()


def test_nothing_else_changes():
    src, X, lists = M.batch(1)
    shape = X.shape[1:]
    B = resident(src, X)
    B.run(B.options(do_n4=False, do_kmeans=False, vox=VOX))
    maps = S.CASES[((83, 75, 9), (41, 37, 9))]
    B.resample_proton(maps)

    def state():
        n4, d, bo, lb, res = B.download(n4=True)
        return (B.download_proton(), B.download_proton_src(), B.download_hp(), B.download_mask().copy(), n4, d, bo, lb,
                np.frombuffer(b"".join(bytes(r) for r in res), np.uint8))

    before = state()
    B.register_maps(M.axis_maps(lists))
    after = state()
    B.close()
    for k, (a, b) in enumerate(zip(before, after)):
        assert same(a, b), k
    assert same(before[1], src) and same(before[2], X)
    assert same(before[0][:2], S.reference_of(src[:2], maps[:2], shape))   # (the studies without NaN: its bits are free)


def test_library_argument_errors():
    """The library's own checks (the binding's are bypassed): VH_ERR_ARG, nothing enqueued or changed, and
    a later valid call still equals the reference."""
    src, X, lists = M.batch(1)
    p, ERR = _lib._ptr, _lib.VH_ERR_ARG
    B = _lib.Batch(41, 37, 9, 4)
    B.upload(X, np.ones(X.shape, np.uint8))
    count = np.asarray([9, 9, 3], np.int32)
    am = np.ascontiguousarray(np.concatenate(M.axis_maps(lists), axis=1))
    score, best, hist = np.zeros((4, 243)), np.zeros((4, 3), np.int32), np.zeros((4, 243, 32, 32), np.uint32)
    call = B.L.vh_batch_register_maps
    assert call(B.h, p(count), p(am), None, p(score), p(best), None, None, None) == ERR         # no resident source
    with pytest.raises(ValueError):
        B.register_maps(M.axis_maps(lists))
    B.upload_proton_src(src)
    assert B.L.vh_batch_download_register_maps_hist(B.h, p(hist)) == ERR                        # before any call
    assert call(None, p(count), p(am), None, p(score), p(best), None, None, None) == ERR
    assert call(B.h, None, p(am), None, p(score), p(best), None, None, None) == ERR
    assert call(B.h, p(count), None, None, p(score), p(best), None, None, None) == ERR
    assert call(B.h, p(count), p(am), None, None, p(best), None, None, None) == ERR
    assert call(B.h, p(count), p(am), None, p(score), None, None, None, None) == ERR
    for bad in ((0, 9, 3), (18, 9, 3), (9, 0, 3), (9, 18, 3), (9, 9, 0), (9, 9, 6), (-1, 9, 3)):
        assert call(B.h, p(np.asarray(bad, np.int32)), p(am), None, p(score), p(best), None, None, None) == ERR, bad
    for at, v in (((0, 0, 0), 4.5), ((3, 20, 0), 0.2), ((1, 5, 1), np.nan), ((2, 12, 1), np.inf), ((3, 20, 1), -2.0 ** 20 - 1),
                  ((0, 9, 0), np.nan)):
        wrong = am.copy()
        wrong[at] = v
        assert call(B.h, p(count), p(wrong), None, p(score), p(best), None, None, None) == ERR, (at, v)
    for home in ((9, 0, 0), (0, 9, 0), (0, 0, 3), (-1, 0, 0)):
        assert call(B.h, p(count), p(am), p(np.asarray(home, np.int32)), p(score), p(best), None, None, None) == ERR, home
        with pytest.raises(ValueError):
            B.register_maps(M.axis_maps(lists), home=home)
    assert B.L.vh_batch_download_register_maps_hist(B.h, p(hist)) == ERR                        # still none
    assert B.L.vh_batch_download_register_maps_hist(B.h, None) == ERR
    assert same(B.download_proton_src(), src) and same(B.download_hp(), X)
    bm, bs, st = np.zeros((4, 3, 2)), np.zeros(4), np.full(4, -1, np.int32)
    assert call(B.h, p(count), p(am), None, p(score), p(best), p(bm), p(bs), p(st)) == _lib.VH_OK   # the nullable three
    assert B.L.vh_batch_download_register_maps_hist(B.h, p(hist)) == _lib.VH_OK
    rh, rs, rbest, _ = M.reference(1)
    assert np.array_equal(hist, rh) and st.tolist() == [0] * 4 and [tuple(b) for b in best] == rbest
    assert np.array_equal(bs, score.max(axis=1))
    for q in range(4):
        assert bm[q].tolist() == [lists[q][a][rbest[q][a]].tolist() for a in range(3)]
    c = B.ctx
    shape = np.asarray(src.shape[1:], np.int64)
    host = c.L.vh_register_maps
    assert host(c.h, None, p(shape), p(X), 41, 37, 9, 4, p(count), p(am), None, p(score), p(best), None, None) == ERR
    assert host(c.h, p(src), None, p(X), 41, 37, 9, 4, p(count), p(am), None, p(score), p(best), None, None) == ERR
    assert host(c.h, p(src), p(shape), None, 41, 37, 9, 4, p(count), p(am), None, p(score), p(best), None, None) == ERR
    assert host(c.h, p(src), p(np.asarray([83, 1025, 9], np.int64)), p(X), 41, 37, 9, 4, p(count), p(am), None, p(score),
                p(best), None, None) == ERR
    assert host(c.h, p(src), p(shape), p(X), 41, 37, 9, 4, p(np.asarray([9, 9, 6], np.int32)), p(am), None, p(score),
                p(best), None, None) == ERR
    B.close()


def test_host_buffer_form_and_class_method():
    from vent_analysis_amd import Vent_Analysis
    src, X, lists = M.batch(1)
    rh, rs, rbest, _ = M.reference(1)
    planted = M.CASES[1][3]
    best, best_map, score, status = _lib.register_maps(src, X, M.axis_maps(lists))
    assert [tuple(b) for b in best] == rbest and status.tolist() == [0] * 4
    assert np.abs(score.reshape(4, -1) - rs).max() <= TOL
    b1, m1, s1, st1 = _lib.register_maps(src[0].astype(np.float64), X[0], lists[0])   # one 3-D volume, its own lists
    assert tuple(b1[0]) == planted[0] and same(s1[0], score[0]) and same(m1[0], best_map[0]) and st1.tolist() == [0]
    # align_proton on study 0: the grids centre on centre at twice the voxel size are case 1's base.  The
    # reference first: the integer registration of the coarse resampling gives a slice (the planted half
    # slice, rounded), the fine lists around the folded map still hold the planted map, and it wins
    va = Vent_Analysis(pickle_dict=dict(HPvent=X[0].copy(), mask=np.ones(X.shape[1:]), vox=list(VOX)))
    keys = set(vars(va))
    va.proton = src[0].astype(np.float64)
    pv = (VOX[0] / 2, VOX[1] / 2, VOX[2])
    shape = X.shape[1:]
    want_map = np.asarray([lists[0][a][planted[0][a]] for a in range(3)])
    m0 = _lib.grid_map(src.shape[1:], pv, shape, VOX)
    shift = G.reference_of(S.resample(src[0], shape, m0)[None], X[:1], (4, 4, 1))[2][0]
    fine, home = _lib.map_candidates(_lib.grid_map(src.shape[1:], pv, shape, VOX, shift), shape, (0.94, 1.0, 1.06))
    _, fs, fbest, _ = M.reference_of(src[:1], X[:1], [fine], home)
    assert shift == (0, 0, 1) and M.gap(fs[0]) >= M.MIN_GAP
    assert same(np.asarray([fine[a][fbest[0][a]] for a in range(3)]), want_map)
    m, value = va.align_proton(pv, factors=(0.94, 1.0, 1.06), apply=False)
    assert same(m, want_map) and value == score[0].max() and same(va.proton, src[0].astype(np.float64))
    m, value = va.align_proton(pv, factors=(0.94, 1.0, 1.06))
    assert same(m, want_map) and value == score[0].max()
    assert same(va.proton, S.resample(src[0], X.shape[1:], want_map))
    assert set(vars(va)) - keys <= {"proton"}                               # no attribute for pickleMe to write
