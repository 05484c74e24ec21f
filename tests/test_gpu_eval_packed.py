"""Every form of eval's walk in one launch (n4_study.hip eval_item), on the windows' bookkeeping a
packed {B_new, B_old} form of it has to keep: the pairs of the column's window shifted and refilled
at a span boundary.  (That form was measured and not kept, DESIGN_LOG.md; the cases stay for the
next attempt at the loop.)

The default four levels with the caps (3, 2, 2, 2) run, in one launch: the call without an old field
(level 0, iteration 1), iterations with both windows on one set of row weights, and at each later
level a first iteration with the old window on the previous level's row tables followed by one on
the level's own.  A second study has a mask of one column: each of its windows moves at every span
boundary.  k_n4_study and k_n4_studyg against the C oracle in both convergence modes, and against
each other and the sweeps bit for bit."""
import functools

import numpy as np
import pytest

import n4_param_cases as P
from test_gpu_n4_params import assert_oracle, assert_same, summary
from test_gpu_parity import _run_one

pytestmark = pytest.mark.gpu

CAPS = (3, 2, 2, 2)
# the threshold far below what three iterations reach: every level runs to its cap
KW = dict(max_iters=CAPS, conv_threshold=1e-7)
STUDIES = ("blob", "column")
SHAPE = "37x45x7"


@functools.lru_cache(maxsize=None)
def case(study):
    X, M = P.volume(SHAPE)
    if study == "column":   # one column (y, z) over all rows
        M = np.zeros_like(M)
        M[:, 22, 3] = 1
        M.setflags(write=False)
    return X, M


@functools.lru_cache(maxsize=None)
def ref(study, conv_mode):
    from oracle import native
    X, M = case(study)
    return native.n4(X, M, conv_mode=conv_mode, **KW)


@functools.lru_cache(maxsize=None)
def gpu(study, driver, conv_mode):
    X, M = case(study)
    return summary(_run_one(X, M, driver, conv_mode=conv_mode, **KW), 4)


@pytest.mark.parametrize("conv_mode", [0, 1])
@pytest.mark.parametrize("driver", ["study", "grid"])
@pytest.mark.parametrize("study", STUDIES)
def test_capped_levels_vs_oracle(study, driver, conv_mode):
    r = ref(study, conv_mode)
    assert list(r[1]) == list(CAPS), r[1]   # every form of the walk runs
    assert_oracle(gpu(study, driver, conv_mode), r, conv_mode, (study, driver))


@pytest.mark.parametrize("study", STUDIES)
def test_capped_levels_drivers_agree_bit_for_bit(study):
    s = gpu(study, "study", 0)
    assert_same(gpu(study, "grid", 0), s, (study, "grid"))
    assert_same(gpu(study, "sweep", 0), s, (study, "sweep"))
