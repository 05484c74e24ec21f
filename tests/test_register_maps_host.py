"""CPU: the host side of the fine registration (vh_axis_candidates, vh_register_maps_pick, the bindings'
argument checks) and the numpy reference against itself: its shared passes against the nested loop of the
spec, the recovery of the planted candidates, and the identity that makes the search a strict
generalisation of the integer window (register_ref)."""
import numpy as np
import pytest

from vent_analysis_amd import _lib

import register_maps_ref as M
import register_ref as G
import resample_ref as S

NEW = ["vh_batch_register_maps", "vh_batch_download_register_maps_hist", "vh_register_maps_pick",
       "vh_axis_candidates", "vh_register_maps"]


def test_symbols_are_exported_and_signed():
    L = _lib.lib()
    for n in NEW:
        assert hasattr(L, n), n
        assert n in _lib._SIGS, n
    assert L.vh_abi_version() == 8


# ---- the candidate formula ----------------------------------------------------------------------------
@pytest.mark.parametrize("base,n_dst", [((2.0, 1.0), 41), ((0.5, -0.25), 37), ((1.3, 7.7), 9), ((1.0, 0.0), 1),
                                        ((3.7, -1000.123), 128)], ids=str)
def test_axis_candidates_equal_the_formula_bit_for_bit(base, n_dst):
    factors, shifts = (0.94, 0.97, 1.0, 1.03, 1.06), (-0.5, 0.0, 0.5, 1.0 / 3.0)
    got = _lib.axis_candidates(base, n_dst, factors, shifts)
    want = M.axis_candidates(base, n_dst, factors, shifts)
    assert got.dtype == np.float64 and got.shape == (20, 2)
    assert got.tobytes() == want.tobytes()
    assert got[2 * 4 + 1].tolist() == [base[0], base[1]]            # factor 1, shift 0: the base itself


def test_axis_candidates_refuse():
    ok = dict(base=(2.0, 1.0), n_dst=41, factors=(1.0,), shifts=(0.0,))
    assert _lib.axis_candidates(**ok).tolist() == [[2.0, 1.0]]
    for bad in (dict(factors=(2.5,)),                               # scale 5
                dict(factors=(0.1,)),                               # scale 0.2
                dict(factors=(float("nan"),)), dict(shifts=(float("inf"),)), dict(shifts=(1e6,)),
                dict(base=(2.0, float("nan"))), dict(n_dst=0), dict(n_dst=(1 << 20) + 1),
                dict(factors=()), dict(shifts=()), dict(base=(2.0,)), dict(factors="ab")):
        with pytest.raises(ValueError):
            _lib.axis_candidates(**{**ok, **bad})
    # the C function itself: null pointers and empty lists, and nothing written on a refusal
    L = _lib.lib()
    f, d, out = np.asarray([1.0, 9.0]), np.asarray([0.0]), np.full((2, 2), -7.0)
    P = _lib._ptr
    assert L.vh_axis_candidates(2.0, 1.0, 41, P(f), 2, P(d), 1, P(out)) == _lib.VH_ERR_ARG
    assert (out == -7.0).all()
    assert L.vh_axis_candidates(2.0, 1.0, 41, None, 2, P(d), 1, P(out)) == _lib.VH_ERR_ARG
    assert L.vh_axis_candidates(2.0, 1.0, 41, P(f), 1, None, 1, P(out)) == _lib.VH_ERR_ARG
    assert L.vh_axis_candidates(2.0, 1.0, 41, P(f), 1, P(d), 1, None) == _lib.VH_ERR_ARG
    assert L.vh_axis_candidates(2.0, 1.0, 41, P(f), 0, P(d), 1, P(out)) == _lib.VH_ERR_ARG
    assert L.vh_axis_candidates(2.0, 1.0, 41, P(f), 1, P(d), 1, P(out)) == _lib.VH_OK and out[0].tolist() == [2.0, 1.0]


def test_map_candidates():
    m = _lib.grid_map((83, 75, 9), (1.0, 1.0, 10.0), (41, 37, 9), (2.0, 2.0, 10.0))
    lists, home = _lib.map_candidates(m, (41, 37, 9))
    assert [l.shape for l in lists] == [(15, 2), (15, 2), (3, 2)] and home == (7, 7, 1)
    for a in range(3):
        assert lists[a][home[a]].tolist() == m[a].tolist()
        assert lists[a].tobytes() == M.axis_candidates(m[a], (41, 37, 9)[a], (1.0,) if a == 2 else _lib.RM_FACTORS,
                                                       _lib.RM_SHIFTS).tobytes()
    lists, home = _lib.map_candidates(m, (41, 37, 9), factors=(0.9, 1.1), shifts=(0.25,), zshifts=(0.0,))
    assert [len(l) for l in lists] == [2, 2, 1] and home == (0, 0, 0)   # no base entry: the middle


# ---- the pick ------------------------------------------------------------------------------------------
def both_picks(score, home=None):
    score = np.asarray(score, np.float64)
    count = (score.shape[1], score.shape[2], score.shape[0])
    got = _lib.register_maps_pick(score, home)
    assert got == M.pick(score, count, home)
    assert got == _lib.register_maps_pick(score.reshape(-1), home, count)
    return got


def test_pick_rules():
    rng = np.random.default_rng(5)
    s = rng.random((3, 5, 4))
    k = np.unravel_index(np.argmax(s), s.shape)
    assert both_picks(s) == (k[1], k[2], k[0])
    # ties: the nearest to home, then the lowest index
    t = np.zeros((3, 5, 5))
    assert both_picks(t) == (2, 2, 1)                               # home is the middle
    assert both_picks(t, (0, 4, 2)) == (0, 4, 2)
    t[1, 2, 2] = -1.0                                               # home itself out: four neighbours at distance 1
    assert both_picks(t) == (2, 2, 0)                               # ... the lowest index is in slice 0
    t[0, 2, 2] = -1.0
    assert both_picks(t) == (1, 2, 1)
    t[:] = 0.0
    t[0, 0, 0] = t[2, 4, 4] = 1.0                                   # equal scores, equal distances: the lowest index
    assert both_picks(t) == (0, 0, 0)
    assert both_picks(t, (3, 3, 1)) == (4, 4, 2)
    # an even list: the middle is (K - 1) // 2
    assert both_picks(np.zeros((2, 4, 2))) == (1, 0, 0)
    # NaN never wins; nothing but NaN gives home
    n = np.full((1, 3, 3), np.nan)
    assert both_picks(n) == (1, 1, 0) and both_picks(n, (2, 0, 0)) == (2, 0, 0)
    n[0, 0, 2] = -5.0
    assert both_picks(n) == (0, 2, 0)
    n[0, 2, 1] = np.inf
    assert both_picks(n) == (2, 1, 0)


def test_pick_refuses():
    for bad in (lambda: _lib.register_maps_pick(np.zeros(9)), lambda: _lib.register_maps_pick(np.zeros((1, 18, 1))),
                lambda: _lib.register_maps_pick(np.zeros((6, 1, 1))), lambda: _lib.register_maps_pick(np.zeros(8), None, (3, 3, 1)),
                lambda: _lib.register_maps_pick(np.zeros((1, 3, 3)), (3, 0, 0)),
                lambda: _lib.register_maps_pick(np.zeros((1, 3, 3)), (0, 0, -1)),
                lambda: _lib.register_maps_pick(np.zeros((1, 3, 3)), (0.0, 0.0, 0.0)),
                lambda: _lib.register_maps_pick(np.zeros(9), None, (3, 3))):
        with pytest.raises(ValueError):
            bad()
    L, P = _lib.lib(), _lib._ptr
    sc, cn, best = np.zeros(9), np.asarray([3, 3, 1], np.int32), np.zeros(3, np.int32)
    assert L.vh_register_maps_pick(None, P(cn), None, P(best)) == _lib.VH_ERR_ARG
    assert L.vh_register_maps_pick(P(sc), None, None, P(best)) == _lib.VH_ERR_ARG
    assert L.vh_register_maps_pick(P(sc), P(cn), None, None) == _lib.VH_ERR_ARG
    assert L.vh_register_maps_pick(P(sc), P(np.asarray([3, 18, 1], np.int32)), None, P(best)) == _lib.VH_ERR_ARG
    assert L.vh_register_maps_pick(P(sc), P(cn), P(np.asarray([0, 3, 0], np.int32)), P(best)) == _lib.VH_ERR_ARG
    assert L.vh_register_maps_pick(P(sc), P(cn), None, P(best)) == _lib.VH_OK and best.tolist() == [1, 1, 0]


# ---- the bindings' checks ------------------------------------------------------------------------------
def test_register_maps_args():
    one = np.asarray([[1.0, 0.0]])
    count, am, home = _lib._register_maps_args([np.asarray([[2.0, 1.0], [2.0, 1.5]]), one, one], 3)
    assert count.dtype == np.int32 and count.tolist() == [2, 1, 1] and home is None
    assert am.dtype == np.float64 and am.shape == (3, 4, 2) and am.flags.c_contiguous
    assert am[2].tolist() == [[2.0, 1.0], [2.0, 1.5], [1.0, 0.0], [1.0, 0.0]]
    per = np.stack([one + q for q in range(3)])                     # one list per study
    count, am, home = _lib._register_maps_args([per, one, one], 3, (0, 0, 0))
    assert am[:, 0, 0].tolist() == [1.0, 2.0, 3.0] and home.dtype == np.int32 and home.tolist() == [0, 0, 0]
    big = np.tile(one, (18, 1))
    for lists, home in (([one, one], None), (np.zeros((3, 1, 2)), None), ([big, one, one], None),
                        ([one, big, one], None), ([one, one, np.tile(one, (6, 1))], None),
                        ([np.zeros((0, 2)), one, one], None), ([np.zeros((1, 3)), one, one], None),
                        ([np.stack([one] * 2), one, one], None),                      # two studies' lists for three
                        ([np.asarray([[4.5, 0.0]]), one, one], None), ([np.asarray([[0.2, 0.0]]), one, one], None),
                        ([one, np.asarray([[1.0, np.nan]]), one], None), ([one, one, np.asarray([[np.inf, 0.0]])], None),
                        ([one, one, np.asarray([[1.0, 2.0 ** 20 + 1]])], None), ([["a", "b"], one, one], None),
                        ([one, one, one], (1, 0, 0)), ([one, one, one], (0, 0, -1)), ([one, one, one], (0, 0)),
                        ([one, one, one], (0.0, 0.0, 0.0))):
        with pytest.raises(ValueError):
            _lib._register_maps_args(lists, 3, home)


# ---- the reference against itself -----------------------------------------------------------------------
def test_shared_passes_equal_the_nested_loop():
    rng = np.random.default_rng(3)
    src = rng.normal(50, 20, (7, 6, 4)).astype(np.float32)
    src[2, 3, 1], src[5, 0, 2] = np.nan, -np.inf
    dst = (5, 4, 3)
    lists = [np.asarray([(1.4, 0.3), (0.8, -0.6), (1.0, 9.0)]), np.asarray([(1.5, 0.0), (0.7, 2.2)]),
             np.asarray([(1.3, 0.1), (1.0, -1.0)])]
    seen = 0
    for kr, kc, kz, Q, counted in M.values(src, dst, lists):
        m = [lists[0][kr], lists[1][kc], lists[2][kz]]
        want, wc = M.value_nested(src, dst, m)
        assert Q.tobytes() == want.tobytes() and Q.tobytes() == S.resample(src, dst, m).tobytes(), (kr, kc, kz)
        assert np.array_equal(counted, wc)
        if kr == 2:
            assert not counted.any()                                # an r map that looks outside the source
        seen += 1
    assert seen == 12


def test_the_reference_recovers_the_planted_candidates():
    _, score, best, status = M.reference(1)
    planted = M.CASES[1][3]
    assert status.tolist() == [0, 0, 0, 0]
    for q, k in enumerate(planted):
        assert best[q] == k, (q, best[q], k)
        assert M.gap(score[q]) >= M.MIN_GAP, (q, M.gap(score[q]))
    assert np.isfinite(score[3]).all()                              # a constant source scores like any other


@pytest.mark.parametrize("shape,search", [((12, 10, 5), (2, 3, 1)), ((9, 11, 3), (4, 1, 2)), ((12, 10, 1), (1, 1, 0))], ids=str)
def test_generalisation_identity(shape, search):
    """A source of the batch's shape, scale 1 and integer offsets -S .. S: the histograms of the integer
    window, candidate (kr, kc, kz) being the shift (kr - Sr, kc - Sc, kz - Sz) -- the two indices run in
    the same order, so the permutation is the identity.  Kinds 0..2: NaN, +-inf and negatives included."""
    P, X = [], []
    for kind in range(3):
        p, x = G.study(shape, (1, -1, 0), kind, 40 + kind)
        P.append(p)
        X.append(x)
    P, X = np.stack(P), np.stack(X)
    lists = [np.asarray([(1.0, float(d)) for d in range(-s, s + 1)]) for s in search]
    hist, score, best, status = M.reference_of(P, X, [lists] * 3)
    whist, wscore, wbest, _ = G.reference_of(P, X, search)
    assert G.shifts(search) == [tuple(k - s for k, s in zip(c, search)) for c in M.candidates([2 * s + 1 for s in search])]
    assert np.array_equal(hist, whist) and hist.sum() > 0
    assert np.array_equal(score, wscore)
    assert [tuple(k - s for k, s in zip(b, search)) for b in best] == wbest
