"""CPU: the host side of the proton-to-xenon registration -- vh_mi and vh_register_pick (no device), the
binding's argument checks, and the numpy reference (register_ref) against the segment reference and
against itself."""
import ctypes as ct

import numpy as np
import pytest

from vent_analysis_amd import _lib

import register_ref as G
import segment_ref as S


def test_symbols_are_exported_and_signed():
    L = _lib.lib()
    for name in ("vh_batch_register", "vh_batch_download_register_hist", "vh_mi", "vh_register_pick", "vh_batch_shift",
                 "vh_batch_download_proton", "vh_register"):
        assert hasattr(L, name) and name in _lib._SIGS, name
    assert L.vh_abi_version() == 8
    assert (_lib.VH_SHIFT_PROTON, _lib.VH_SHIFT_MASK) == (0, 1)


def test_mi_equals_the_numpy_formula():
    """1e-10 absolute: at most 1024 terms, |log| <= ln(1.6e11) ~ 26, a few ulp each, divided by n."""
    rng = np.random.default_rng(5)
    hists = [rng.integers(0, 50, (32, 32)), rng.integers(0, 400000, (32, 32)),
             (rng.random((32, 32)) < 0.1) * rng.integers(1, 1000, (32, 32)),
             np.diag(rng.integers(1, 100, 32)), rng.integers(0, 9, (5, 5)), np.full((32, 32), 393216 // 4)]
    hists += [G.reference((41, 37, 9), (4, 4, 2))[0][q, i] for q in range(3) for i in (0, 202, 404)]
    for h in hists:
        h = np.asarray(h, np.uint32)
        got, want = _lib.mi(h), G.mi(h)
        assert isinstance(got, float) and abs(got - want) <= 1e-10, (got, want)
    assert _lib.mi(np.diag(np.full(32, 7))) == pytest.approx(np.log(32.0), abs=1e-12)   # a bijection: ln(levels)


def test_mi_is_exactly_zero_for_degenerate_histograms():
    rng = np.random.default_rng(6)
    row, col = np.zeros((32, 32), np.uint32), np.zeros((32, 32), np.uint32)
    row[7] = rng.integers(0, 100000, 32)
    col[:, 31] = rng.integers(0, 100000, 32)
    for h in (row, col, np.zeros((32, 32), np.uint32)):
        assert _lib.mi(h) == 0.0 and G.mi(h) == 0.0
    one = np.zeros((32, 32), np.uint32)
    one[0, 0] = 393216
    assert _lib.mi(one) == 0.0
    with pytest.raises(ValueError):
        _lib.mi(np.zeros((32, 31), np.uint32))
    with pytest.raises(ValueError):
        _lib.mi(np.zeros(32, np.uint32))
    L = _lib.lib()
    out = ct.c_double(0)
    assert L.vh_mi(None, 32, ct.byref(out)) == _lib.VH_ERR_ARG
    assert L.vh_mi(_lib._ptr(one), 0, ct.byref(out)) == _lib.VH_ERR_ARG
    assert L.vh_mi(_lib._ptr(one), 32, None) == _lib.VH_ERR_ARG


def _scores(search, fill=0.0):
    return np.full((2 * search[2] + 1, 2 * search[0] + 1, 2 * search[1] + 1), fill, np.float64)


def test_the_pick_rule():
    search = (2, 3, 1)
    sc = _scores(search)
    assert _lib.register_pick(sc, search) == G.pick(sc, search) == (0, 0, 0)        # all equal
    sc[2, 4, 0] = 1.0                                                                # (dz, dr, dc) = (1, 2, -3)
    assert _lib.register_pick(sc, search) == G.pick(sc, search) == (2, -3, 1)
    sc[1, 2, 5] = 1.0                                                                # (0, 0, 2): L1 2 beats L1 6
    assert _lib.register_pick(sc, search) == G.pick(sc, search) == (0, 2, 0)
    sc[1, 1, 2] = sc[1, 2, 4] = sc[0, 2, 3] = 1.0       # (-1, -1, 0) of L1 2; (0, 1, 0) and (0, 0, -1) of L1 1
    # among the two of L1 1 the lower index wins: dz is the slowest axis
    assert _lib.register_pick(sc, search) == G.pick(sc, search) == (0, 0, -1)
    sc[1, 2, 3] = 1.0                                                                # the centre ties: L1 0
    assert _lib.register_pick(sc, search) == (0, 0, 0)
    sc[0, 0, 0] = 1.0 + 1e-15                                                        # a larger score beats any norm
    assert _lib.register_pick(sc, search) == G.pick(sc, search) == (-2, -3, -1)
    assert _lib.register_pick(sc.reshape(-1), search) == (-2, -3, -1)               # flat, in index order
    nan = _scores(search, np.nan)
    assert _lib.register_pick(nan, search) == G.pick(nan, search) == (0, 0, 0)
    nan[2, 0, 1] = -5.0                                                              # a NaN never wins
    assert _lib.register_pick(nan, search) == G.pick(nan, search) == (-2, -2, 1)
    rng = np.random.default_rng(8)
    for search in ((0, 0, 0), (8, 8, 2), (1, 0, 2), (4, 4, 1)):
        sc = np.round(rng.random(_scores(search).shape), 1)                          # many ties
        assert _lib.register_pick(sc, search) == G.pick(sc, search)
    with pytest.raises(ValueError):
        _lib.register_pick(np.zeros(5), (1, 1, 0))
    L = _lib.lib()
    best = np.zeros(3, np.int32)
    p = _lib._ptr
    assert L.vh_register_pick(None, p(np.array([1, 1, 0], np.int32)), p(best)) == _lib.VH_ERR_ARG
    assert L.vh_register_pick(p(np.zeros(9)), None, p(best)) == _lib.VH_ERR_ARG
    assert L.vh_register_pick(p(np.zeros(9)), p(np.array([9, 0, 0], np.int32)), p(best)) == _lib.VH_ERR_ARG
    assert L.vh_register_pick(p(np.zeros(9)), p(np.array([1, 1, 0], np.int32)), None) == _lib.VH_ERR_ARG


def test_argument_checks_run_before_any_device_call():
    shape = (41, 37, 9)
    assert _lib._register_args((4, 4, 1), shape).tolist() == [4, 4, 1]
    assert _lib._register_args(np.array([8, 8, 2]), shape).dtype == np.int32
    for bad in ((9, 0, 0), (0, 9, 0), (0, 0, 3), (-1, 0, 0), (0, -1, 0), (0, 0, -1), (4, 4), (4, 4, 1, 0), 4,
                (4.0, 4.0, 1.0), (True, False, True), None):
        with pytest.raises(ValueError):
            _lib._register_args(bad, shape)
    for bad, small in (((8, 0, 0), (8, 37, 9)), ((0, 8, 0), (41, 8, 9)), ((0, 0, 1), (41, 37, 1)), ((2, 0, 0), (2, 37, 9))):
        with pytest.raises(ValueError):
            _lib._register_args(bad, small)
    assert _lib._register_args((7, 7, 0), (8, 8, 1)).tolist() == [7, 7, 0]
    assert _lib._shift_args((1, -2, 0), 3, shape).tolist() == [[1, -2, 0]] * 3
    assert _lib._shift_args([(41, -37, 9)] * 2, 2, shape).dtype == np.int32
    for bad in ((42, 0, 0), (0, -38, 0), (0, 0, 10), (1, 2), [(1, 2, 3)] * 2, (1.0, 0.0, 0.0)):
        with pytest.raises(ValueError):
            _lib._shift_args(bad, 3, shape)
    # the module-level call and the class method refuse before they touch a context
    x = np.ones((8, 8, 2), np.float32)
    with pytest.raises(ValueError):
        _lib.register(x, x, (9, 0, 0), device=10 ** 6)
    with pytest.raises(ValueError):
        _lib.register(x, np.ones((8, 8, 3), np.float32), (1, 1, 0), device=10 ** 6)
    from vent_analysis_amd import Vent_Analysis
    va = Vent_Analysis(pickle_dict=dict(HPvent=np.ones(shape, np.float32), mask=np.ones(shape), vox=[1.5, 1.5, 10.0]))
    with pytest.raises(ValueError):
        va.register_proton()                       # no proton
    va.proton = np.ones((41, 37, 8))
    with pytest.raises(ValueError):
        va.register_proton()                       # another shape
    va.proton = np.ones(shape)
    with pytest.raises(ValueError):
        va.register_proton(search=(0, 0, 3))
    assert _lib.lib().vh_batch_register(None, None, None, None, None, None) == _lib.VH_ERR_ARG
    assert _lib.lib().vh_batch_shift(None, 0, None) == _lib.VH_ERR_ARG


@pytest.mark.parametrize("shape", [(41, 37, 9), (12, 10, 1)], ids=str)
def test_joint_at_shift_zero_folds_the_segment_histogram(shape):
    """With every xenon voxel valid, the row sums of J at shift 0 are the proton's 256-bin histogram of
    the segment statistics folded by 8 -- the same bins, the same maximum."""
    P, X = G.batch(shape)
    for q in (0, 1, 2, 3):
        x = X[0] if q == 2 else X[q]                # (study 2's xenon is salted: take a clean one)
        cp, cx = G.codes(P[q]), G.codes(x)
        assert (cx != G.INVALID).all()
        J = G.joint(cp, cx, (0, 0, 0))
        pmax, h256 = S.stats(P[q])
        assert pmax == G.image_max(P[q])
        assert np.array_equal(J.sum(axis=1), h256.reshape(32, 8).sum(axis=1))
        assert int(J.sum()) == int((cp != G.INVALID).sum())


def test_the_reference_itself():
    shape, search, planted = G.CASES[0]
    P, X = G.batch(shape)
    hist, score, best, gaps = G.reference(shape, search)
    sh = G.shifts(search)
    assert len(sh) == 9 * 9 * 5 and sh[0] == (-4, -4, -2) and sh[((1 + 2) * 9 + (3 + 4)) * 9 + (-2 + 4)] == (3, -2, 1)
    assert all(g >= 1e-6 for g in gaps[:3]) and best[:3] == planted and best[3] == (0, 0, 0)
    assert (score[3] == 0.0).all()                                       # a constant proton
    zero_bin = hist[1, sh.index((0, 0, 0))]
    assert zero_bin[0, 0] > zero_bin.sum() // 2                          # study 1: one bin holds most pairs
    # a voxel pair at a time, on a small crop
    cp, cx = G.codes(P[2]), G.codes(X[2])
    s = (2, -3, 1)
    J = np.zeros((32, 32), np.uint32)
    for r in range(41):
        for c in range(37):
            for z in range(9):
                r2, c2, z2 = r + s[0], c + s[1], z + s[2]
                if 0 <= r2 < 41 and 0 <= c2 < 37 and 0 <= z2 < 9 and cp[r2, c2, z2] != 255 and cx[r, c, z] != 255:
                    J[cp[r2, c2, z2], cx[r, c, z]] += 1
    assert np.array_equal(J, hist[2, sh.index(s)])
    # codes: the invalid voxels, -0.0, the maximum
    x = np.array([[[0.0, -0.0, 1.0, 2.0, np.nan, np.inf, -np.inf, -1.0, 1.99, 0.0078125]]], np.float32)
    assert G.codes(x).reshape(-1).tolist() == [0, 0, 16, 31, 255, 255, 255, 255, 31, 0]
    assert G.codes(np.zeros((2, 2, 2))) is None and G.codes(np.full((2, 2, 2), -1.0)) is None
    # the shift: zeros come in, the rest moves
    a = np.arange(2 * 3 * 4 * 5).reshape(2, 3, 4, 5) + 1
    b = G.shift_image(a, (1, -2, 0))
    assert b[1, 0, 2, 3] == a[1, 1, 0, 3] and (b[:, 2] == 0).all() and (b[:, :, :2] == 0).all()
    assert np.array_equal(G.shift_image(a, (0, 0, 0)), a) and not G.shift_image(a, (3, 0, 0)).any()
