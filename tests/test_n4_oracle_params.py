"""The C oracle (oracle/n4_oracle.c) off the N4 defaults: what test_gpu_n4_params.py rests on.  A case
that stopped changing the oracle's output, or that ran one iteration per level, would make its GPU
twin vacuous; the prefix and threshold properties asserted of the device hold of the reference."""
import numpy as np
import pytest

import n4_param_cases as P

TABLE = P.table()
IDS = [f"{c}-{s}" for c, s in TABLE]


@pytest.mark.parametrize("conv_mode", [0, 1])
@pytest.mark.parametrize("case,shape", TABLE, ids=IDS)
def test_case_is_finite_bounded_and_off_the_default(case, shape, conv_mode):
    kw = P.params(case)
    out, its, conv = P.oracle(shape, case, conv_mode)
    caps = kw.get("max_iters", P.FOUR)
    assert len(its) == len(conv) == len(caps)
    assert np.isfinite(out).all() and np.isfinite(conv).all()
    assert all(1 <= i <= c for i, c in zip(its, caps)), (list(its), caps)
    assert max(its) > 1                       # the loop ran on at least one level
    base = P.oracle(shape, "default", conv_mode)[0]
    _, M = P.volume(shape)
    assert (out != base)[M > 0].any()         # the parameter reaches the field


@pytest.mark.parametrize("shape", P.MAIN_SHAPES)
def test_cap_case_stops_at_its_caps(shape):
    """(7, 1, 3, 2): the levels that would run longer stop at the cap, with a convergence value still
    above the threshold on the levels that did not converge."""
    _, its, conv = P.oracle(shape, "cap")
    free = P.oracle(shape, "default")[1]
    assert its[0] == 7 < free[0] and conv[0] > 0.001
    assert its[1] == 1


@pytest.mark.parametrize("conv_mode", [0, 1])
@pytest.mark.parametrize("shape", list(P.SHAPES))
def test_prefix_property(shape, conv_mode):
    """Levels run in sequence from the same state: the first k levels of the four-level run are the
    k-level run, bit for bit."""
    _, its4, conv4 = P.oracle(shape, "default", conv_mode)
    for k in (1, 2, 3):
        _, its, conv = P.oracle(shape, P.PREFIX[k], conv_mode)
        assert list(its) == list(its4[:k]), (k, list(its), list(its4))
        assert conv.tobytes() == conv4[:k].tobytes(), (k, conv, conv4)


@pytest.mark.parametrize("conv_mode", [0, 1])
@pytest.mark.parametrize("shape", list(P.SHAPES))
def test_level0_iterations_grow_as_the_threshold_falls(shape, conv_mode):
    """Level 0 follows one trajectory whatever the threshold; it stops at the first iteration whose
    convergence value is below it."""
    hi, mid, lo = (P.oracle(shape, c, conv_mode) for c in P.THRESHOLDS)
    assert hi[1][0] <= mid[1][0] <= lo[1][0]
    assert hi[1][0] < lo[1][0]
    assert hi[2][0] < 0.003 and mid[2][0] < 0.001 and lo[2][0] < 3e-4
    assert hi[2][0] >= mid[2][0] >= lo[2][0]
