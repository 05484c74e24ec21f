"""N4 off its defaults on the three drivers (the per-iteration sweeps, k_n4_study, k_n4_studyg): the
control lattice per axis, the level count and caps, the convergence threshold, the deconvolution's
width and noise, the bin count, and the sweep driver's sub-batches, each against the C oracle
(oracle.native.n4 with the same keywords, pinned off the defaults by test_n4_oracle_params.py) under
assert_n4_matches: identical iteration counts, float32-identical convergence values for conv_mode 0
and rtol 1e-9 for conv_mode 1, the field within 1 ulp.

The volumes are the smallest the drivers take different paths on: 37x45x7 (odd sizes, five 64-column
tiles, one row slot), 24x20x6 (two tiles) and, for the lattice cases, 12x70x9 (ten tiles, a column
range over one tile in a single row slot).  A run of (shape, case, driver, conv_mode) is made once
and shared by the tests that read it."""
import functools

import numpy as np
import pytest

from vent_analysis_amd import _lib
from vent_analysis_amd.synth import synth_batch

import n4_param_cases as P
from test_gpu_parity import _run_batch, _run_one, assert_n4_matches

pytestmark = pytest.mark.gpu

DRIVERS = ("sweep", "study", "grid")
VOX = (1.5, 1.5, 10.0)
TABLE = P.table()
IDS = [f"{c}-{s}" for c, s in TABLE]


def f32_bytes(v):
    return np.asarray(v, np.float32).tobytes()


def summary(out, nl, b=0):
    """One study of a download: (field, defect, border, LB map, iterations, convergence values)."""
    n4, d, bo, lb, res = out
    return n4[b], d[b], bo[b], lb[b], list(res[b].n4_iters[:nl]), list(res[b].n4_conv[:nl])


def assert_same(a, b, tag):
    """Two summaries, bit for bit."""
    assert a[4] == b[4], (tag, a[4], b[4])
    assert f32_bytes(a[5]) == f32_bytes(b[5]), (tag, a[5], b[5])
    assert a[0].tobytes() == b[0].tobytes(), (tag, "field")
    for k, name in ((1, "defect"), (2, "border"), (3, "lb")):
        assert np.array_equal(a[k], b[k]), (tag, name)


def assert_oracle(s, ref, conv_mode, tag):
    assert_n4_matches(s[0], s[4], s[5], *ref, conv_mode, tag)


@functools.lru_cache(maxsize=None)
def _gpu(shape, case, driver, conv_mode):
    X, M = P.volume(shape)
    kw = P.params(case)
    return summary(_run_one(X, M, driver, conv_mode=conv_mode, **kw), P.n_levels(kw))


def gpu(shape, case, driver, conv_mode=0):
    """The study of a shape through one driver (an "LDS budget" refusal raises: the test fails)."""
    return _gpu(shape, case, driver, conv_mode)


# ---- the case table ------------------------------------------------------------------------------------
@pytest.mark.parametrize("conv_mode", [0, 1])
@pytest.mark.parametrize("driver", DRIVERS)
@pytest.mark.parametrize("case,shape", TABLE, ids=IDS)
def test_case_vs_oracle(case, shape, driver, conv_mode):
    s = gpu(shape, case, driver, conv_mode)
    ref = P.oracle(shape, case, conv_mode)
    assert_oracle(s, ref, conv_mode, (case, shape, driver))
    if case == "cap":   # a level the oracle stops at its cap stops there on the device
        caps = P.params(case)["max_iters"]
        assert any(o == c for o, c in zip(ref[1], caps))
        assert all(g == c for g, o, c in zip(s[4], ref[1], caps) if o == c), (s[4], caps)


@pytest.mark.parametrize("case,shape", TABLE, ids=IDS)
def test_drivers_agree_bit_for_bit(case, shape):
    """study = grid = sweep under conv_mode 0: the same S1-S9 operations, so the same field,
    iteration counts, convergence values and maps."""
    s = gpu(shape, case, "sweep")
    for driver in ("study", "grid"):
        assert_same(gpu(shape, case, driver), s, (case, shape, driver))


@pytest.mark.parametrize("driver", DRIVERS)
@pytest.mark.parametrize("shape", P.MAIN_SHAPES)
def test_prefix_property(shape, driver):
    """The levels run in sequence from the same state: the k-level run of max_iters (50,) * k gives
    the first k iteration counts and convergence values of the four-level run, bit for bit."""
    full = gpu(shape, P.PREFIX[4], driver)
    assert_oracle(full, P.oracle(shape, P.PREFIX[4]), 0, (shape, driver, 4))
    for k in (1, 2, 3):
        s = gpu(shape, P.PREFIX[k], driver)
        assert s[4] == full[4][:k], (shape, driver, k, s[4], full[4])
        assert f32_bytes(s[5]) == f32_bytes(full[5][:k]), (shape, driver, k, s[5], full[5])
        assert_oracle(s, P.oracle(shape, P.PREFIX[k]), 0, (shape, driver, k))


@pytest.mark.parametrize("conv_mode", [0, 1])
@pytest.mark.parametrize("driver", DRIVERS)
@pytest.mark.parametrize("shape", P.MAIN_SHAPES)
def test_level0_iterations_grow_as_the_threshold_falls(shape, driver, conv_mode):
    """Level 0 follows one trajectory whatever the threshold: its count at 0.003 is at most that at
    0.001, which is at most that at 3e-4, and each is the oracle's."""
    its = []
    for case in P.THRESHOLDS:
        s = gpu(shape, case, driver, conv_mode)
        assert s[4][0] == P.oracle(shape, case, conv_mode)[1][0], (shape, driver, case)
        its.append(s[4][0])
    assert its[0] <= its[1] <= its[2], its


# ---- the cases the volume-resident kernels may refuse -------------------------------------------------
def second_study(shape):
    """A batch of two: the shape's study and a neighbour of it (another seed)."""
    R, C, Z, seed = P.SHAPES[shape]
    hp, mk = synth_batch(R, C, Z, 2, base_seed=seed)
    return hp, mk.astype(np.uint8)


def run_on(B, mode, nl, **kw):
    B.run(B.options(do_n4=True, vox=VOX, n4_mode=mode, **kw))
    out = B.download(n4=True)
    return [summary(out, nl, b) for b in range(B.shape[0])]


def large_case(shape, kw, conv_mode):
    """sweep and auto (a batch of one, a batch of two) run and match the oracle; study and grid match
    it or refuse by the LDS budget, and after a refusal the same Batch runs the defaults."""
    from oracle import native
    nl = P.n_levels(kw)
    X, M = P.volume(shape)
    R, C, Z = X.shape
    hp, mk = second_study(shape)
    refs = [native.n4(hp[b], mk[b], conv_mode=conv_mode, **kw) for b in range(2)]
    ref1 = native.n4(X, M, conv_mode=conv_mode, **kw)
    sweep = summary(_run_one(X, M, "sweep", conv_mode=conv_mode, **kw), nl)
    assert_oracle(sweep, ref1, conv_mode, (shape, "sweep"))
    auto = summary(_run_one(X, M, "auto", conv_mode=conv_mode, **kw), nl)
    assert_oracle(auto, ref1, conv_mode, (shape, "auto", 1))
    for mode in ("sweep", "auto"):
        out = _run_batch(hp, mk, mode, conv_mode=conv_mode, **kw)
        for b in range(2):
            assert_oracle(summary(out, nl, b), refs[b], conv_mode, (shape, mode, 2, b))
    refused = {}
    for mode in ("study", "grid"):
        B = _lib.Batch(R, C, Z, 1)
        try:
            B.upload(X[None], M[None])
            try:
                s = run_on(B, mode, nl, conv_mode=conv_mode, **kw)[0]
            except ValueError as e:
                assert "LDS budget" in str(e), (shape, mode, str(e))
                refused[mode] = str(e)
                s = run_on(B, mode, 4, conv_mode=conv_mode)[0]   # the batch still runs the defaults
                assert_oracle(s, P.oracle(shape, "default", conv_mode), conv_mode, (shape, mode, "after"))
                if conv_mode == 0:
                    assert_same(s, gpu(shape, "default", mode), (shape, mode, "after"))
            else:
                assert_oracle(s, ref1, conv_mode, (shape, mode))
                if conv_mode == 0:
                    assert_same(s, sweep, (shape, mode))
        finally:
            B.close()
    return refused


@pytest.mark.parametrize("conv_mode", [0, 1])
@pytest.mark.parametrize("shape", P.MAIN_SHAPES)
def test_ncp_777_four_levels(shape, conv_mode):
    """ncp (7, 7, 7), four levels: final lattice 35^3.  The sweeps run it; k_n4_study and k_n4_studyg
    refuse it at both shapes (study_layout asks 914 KB of the 160 KB: the fit's two 64-bit numerators
    per control point, 16 B x 42875, then the float lattice and its refinement copies)."""
    large_case(shape, P.LARGE["ncp-777"], conv_mode)


@pytest.mark.parametrize("conv_mode", [0, 1])
@pytest.mark.parametrize("shape", P.MAIN_SHAPES)
def test_five_levels(shape, conv_mode):
    """max_iters (8, 8, 8, 8, 8): final lattice 19^3.  The sweeps run it; the volume-resident kernels
    refuse it at both shapes by 7 KB (171200 B at 37x45x7, 170992 B at 24x20x6, of 163840: the fit's
    numerators are 109744 B of it, its ring rows 24 KB, the lattice 27 KB)."""
    large_case(shape, P.LARGE["levels-5"], conv_mode)


SIX = P.LARGE["levels-8"]["max_iters"][:6]


@pytest.mark.parametrize("mode,nb", [("sweep", 1), ("sweep", 2), ("auto", 1), ("auto", 2), ("study", 1),
                                     ("grid", 1)])
def test_eight_levels_is_past_the_row_lattice_limit(mode, nb):
    """max_iters (3, 3, 3, 3, 2, 2, 2, 2), VH_MAX_LEVELS levels: no driver takes it.  With ncp 4 the
    lattice has 2^L + 3 control points per axis at level L, and every driver's fit holds a tile's
    control rows in one wave's lanes: at most 64 along the rows (vh_ensure_n4_workspace), so 67 at
    the seventh level and 131 at the eighth are refused for every ncp >= 4, whatever the shape.  The
    limit found: six levels (35 control points) is the most a run can have; test_six_levels runs
    it.  The refusal is the argument error, and the batch runs the defaults afterwards."""
    shape = "37x45x7"
    hp, mk = second_study(shape)
    hp, mk = hp[:nb], mk[:nb]
    B = _lib.Batch(*hp.shape[1:], nb)
    try:
        B.upload(hp, mk)
        for iters in (P.LARGE["levels-8"]["max_iters"], P.LARGE["levels-8"]["max_iters"][:7]):
            with pytest.raises(ValueError, match="N4 lattice too fine: > 64 control points along rows"):
                run_on(B, mode, len(iters), max_iters=iters)
        got = run_on(B, mode, 4)
        assert_oracle(got[0], P.oracle(shape, "default"), 0, (mode, nb, "after"))
        assert_same(got[0], gpu(shape, "default", "sweep"), (mode, nb, "after"))
    finally:
        B.close()


@pytest.mark.parametrize("conv_mode", [0, 1])
@pytest.mark.parametrize("shape", P.MAIN_SHAPES)
def test_six_levels(shape, conv_mode):
    """max_iters (3, 3, 3, 3, 2, 2): the largest level count any driver accepts (final lattice 35^3;
    see test_eight_levels_is_past_the_row_lattice_limit).  The sweeps run it; the volume-resident
    kernels refuse it as they refuse ncp (7, 7, 7) with four levels, the same lattice."""
    large_case(shape, dict(max_iters=SIX), conv_mode)


BAD = [dict(max_iters=(2,) * 9), dict(ncp=(3, 4, 4)), dict(n_bins=1), dict(n_bins=257)]


@pytest.mark.parametrize("mode,nb", [("sweep", 2), ("study", 2), ("grid", 1), ("auto", 1)])
def test_argument_errors_leave_the_batch_usable(mode, nb):
    """Nine levels, ncp below 4, n_bins outside 2..256: check_n4_params's argument error on every
    driver, before anything is launched; the batch then runs the defaults."""
    shape = "24x20x6"
    hp, mk = second_study(shape)
    hp, mk = hp[:nb], mk[:nb]
    B = _lib.Batch(*hp.shape[1:], nb)
    try:
        B.upload(hp, mk)
        for kw in BAD:
            with pytest.raises(ValueError, match="unsupported N4 parameters"):
                B.run(B.options(do_n4=True, vox=VOX, n4_mode=mode, **kw))
        got = run_on(B, mode, 4)
        assert_oracle(got[0], P.oracle(shape, "default"), 0, (mode, "after"))
        assert_same(got[0], gpu(shape, "default", "sweep"), (mode, "after"))
    finally:
        B.close()


# ---- one Batch across a change of the lattice ----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pair():
    hp, mk = second_study("37x45x7")
    hp.setflags(write=False)
    mk.setflags(write=False)
    return hp, mk


@functools.lru_cache(maxsize=None)
def pair_ref(b, case, conv_mode):
    from oracle import native
    hp, mk = pair()
    return native.n4(hp[b], mk[b], conv_mode=conv_mode, **P.params(case))


@pytest.mark.parametrize("conv_mode", [0, 1])
@pytest.mark.parametrize("mode,nb", [("sweep", 2), ("study", 2), ("grid", 1)])
def test_workspace_across_a_parameter_change(mode, nb, conv_mode):
    """One Batch through the defaults (lattice 11^3), ncp (5, 6, 4) with three levels (11x15x7: P1
    grows, the lattice stride stays larger than needed), ncp (4, 4, 5) (11x11x19: the lattice buffers
    are allocated again) and the defaults again: every run equals the oracle and, bit for bit, the same
    run on a fresh Batch."""
    hp, mk = (a[:nb] for a in pair())
    B = _lib.Batch(37, 45, 7, nb)
    try:
        B.upload(hp, mk)
        for run, case in enumerate(("default", "ncp-564", "ncp-z", "default")):
            kw = P.params(case)
            nl = P.n_levels(kw)
            got = run_on(B, mode, nl, conv_mode=conv_mode, **kw)
            out = _run_batch(hp, mk, mode, conv_mode=conv_mode, **kw)
            for b in range(nb):
                assert_oracle(got[b], pair_ref(b, case, conv_mode), conv_mode, (mode, run, case, b))
                assert_same(got[b], summary(out, nl, b), (mode, run, case, b))
    finally:
        B.close()


# ---- auto at a batch of 16 or more ---------------------------------------------------------------------
def test_auto_takes_the_study_kernel_off_the_defaults():
    """17 studies of 24x20x6 with ncp (5, 4, 4): n4_mode auto takes k_n4_study (nb >= 16 and the state
    fits: "study" does not refuse it) and equals the sweeps bit for bit; a study with an empty mask
    comes back untouched."""
    from oracle import native
    kw = dict(ncp=(5, 4, 4))
    hp, mk = synth_batch(24, 20, 6, 17, base_seed=50)
    mk = mk.astype(np.uint8)
    mk[5] = 0
    auto = _run_batch(hp, mk, "auto", **kw)
    for mode in ("sweep", "study"):
        other = _run_batch(hp, mk, mode, **kw)
        for b in range(17):
            assert_same(summary(auto, 4, b), summary(other, 4, b), (mode, b))
    for b in (0, 8, 16):
        assert_oracle(summary(auto, 4, b), native.n4(hp[b], mk[b], **kw), 0, ("auto", b))
    assert auto[4][5].n_mask == 0 and not auto[1][5].any()
    assert np.array_equal(auto[0][5], hp[5])
    assert list(auto[4][5].n4_iters[:4]) == [0, 0, 0, 0]


# ---- the other entry points ----------------------------------------------------------------------------
def test_host_entry_point_off_the_defaults():
    """vh_n4 (_lib.n4) with the combo parameters: what the resident batch computes, bit for bit."""
    shape = "37x45x7"
    X, M = P.volume(shape)
    out, its, conv = _lib.n4(X, M, **P.params("combo"))
    s = gpu(shape, "combo", "sweep")
    assert list(its[0]) == s[4] and f32_bytes(conv[0]) == f32_bytes(s[5])
    assert out[0].tobytes() == s[0].tobytes()
    assert_n4_matches(out[0], its[0], conv[0], *P.oracle(shape, "combo"), 0, "vh_n4")


def test_pipe_off_the_defaults():
    """vh_pipe with ragged sub-batches (5 studies, 2 per sub-batch, 2 slots) and the combo parameters:
    what one resident batch of the five computes, bit for bit."""
    kw = P.params("combo")
    hp, mk = synth_batch(37, 45, 7, 5, base_seed=11)
    mk = mk.astype(np.uint8)
    B = _lib.Batch(37, 45, 7, 5)
    B.upload(hp, mk)
    o = B.options(do_n4=True, vox=VOX, **kw)
    B.run(o)
    ref = B.download(n4=True)
    B.close()
    pipe = _lib.Pipe(37, 45, 7, 2, slots=2)
    got = pipe.run(hp, mk, o)
    pipe.close()
    for b in range(5):
        assert_same(summary(got, 3, b), summary(ref, 3, b), ("pipe", b))
    assert_oracle(summary(got, 3, 0), P.oracle("37x45x7", "combo"), 0, "pipe")
    assert any(sum(r.n4_iters[:3]) > 3 for r in got[4])


# ---- sub-batches of the sweep driver -------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{}, dict(ncp=(4, 6, 4))], ids=["default", "ncp-y"])
def test_sweep_subbatches(kw, monkeypatch):
    """vh_launch_n4's sub-batch loop: five studies (the third with an empty mask) in sub-batches of 1,
    2, 3, 5 and 7 (more than the batch) give what the whole batch in one gives, bit for bit, twice
    over on one Batch in an order in which the sub-batch shrinks and grows."""
    from oracle import native
    monkeypatch.delenv("VH_N4_SUBBATCH", raising=False)
    hp, mk = synth_batch(37, 45, 7, 5, base_seed=11)
    mk = mk.astype(np.uint8)
    mk[2] = 0
    whole = _run_batch(hp, mk, "sweep", n4_subbatch=0, **kw)
    base = [summary(whole, 4, b) for b in range(5)]
    for b in (0, 1, 3, 4):
        assert_oracle(base[b], native.n4(hp[b], mk[b], **kw), 0, ("whole", b))
    assert np.array_equal(base[2][0], hp[2]) and base[2][4] == [0, 0, 0, 0] and not base[2][1].any()
    B = _lib.Batch(37, 45, 7, 5)
    try:
        B.upload(hp, mk)
        for rnd in range(2):
            for sub in (2, 5, 1, 7, 3):
                got = run_on(B, "sweep", 4, n4_subbatch=sub, **kw)
                for b in range(5):
                    assert_same(got[b], base[b], (rnd, sub, b))
    finally:
        B.close()
