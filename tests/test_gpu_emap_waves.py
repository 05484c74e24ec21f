"""The E map of the volume-resident N4 kernels (k_n4_study, k_n4_studyg: emap_phase) against the sweep
driver's k_n4_emap, an independent GPU restatement of the same arithmetic, and against the C oracle.

The E map depends on the bin count, the kernel width, the noise and the histogram, not on the
volume's size, so the volumes are tiny: 16 studies of 16x16x4 with per-study lung geometry for the
study form, one such study for the grid form.  The bin counts move the series' pad offset
(512 - bins) / 2 over even and odd values (156, 231, 128 with one pad slot more behind the series
than before it, 128) and reach the largest count; one case has a two-level schedule."""
import functools

import numpy as np
import pytest

from oracle import native
from vent_analysis_amd.synth import synth_batch
from test_gpu_parity import _run_batch, assert_n4_matches

pytestmark = pytest.mark.gpu

SHAPE, NB = (16, 16, 4), 16
# (n_bins, max_iters): the default schedule, and one of two levels
CASES = [(200, (50, 50, 50, 50)), (50, (50, 50, 50, 50)), (255, (50, 50, 50, 50)),
         (256, (50, 50, 50, 50)), (200, (8, 5))]
IDS = ["bins200", "bins50", "bins255", "bins256", "bins200-two-levels"]


@functools.lru_cache(maxsize=None)
def batch():
    hp, mk = synth_batch(*SHAPE, NB, base_seed=40, vary=True)
    assert all(int(m.sum()) >= 2 for m in mk)   # every study runs the loop
    hp.setflags(write=False)
    mk.setflags(write=False)
    return hp, mk


@functools.lru_cache(maxsize=None)
def sweep(bins, iters):
    """The batch through the sweep driver (k_n4_emap): (N4 volumes, iterations, convergence values)."""
    return summary(_run_batch(*batch(), "sweep", n_bins=bins, max_iters=iters), len(iters))


def summary(out, nlev):
    n4, res = out[0], out[4]
    return (n4, [list(r.n4_iters[:nlev]) for r in res], [list(r.n4_conv[:nlev]) for r in res])


def assert_same(got, ref, studies, tag):
    for b in studies:
        assert got[1][b] == ref[1][b], (tag, b, got[1][b], ref[1][b])
        assert got[2][b] == ref[2][b], (tag, b, got[2][b], ref[2][b])
        assert got[0][b].tobytes() == ref[0][b].tobytes(), (tag, b)


def assert_oracle(got, hp, mk, studies, bins, iters, tag):
    for b in studies:
        ref, its_ref, conv_ref = native.n4(hp[b], mk[b], n_bins=bins, max_iters=iters)
        assert_n4_matches(got[0][b], got[1][b], got[2][b], ref, its_ref, conv_ref, 0, (tag, b))


@pytest.mark.parametrize("bins,iters", CASES, ids=IDS)
def test_study_form_equals_sweeps_and_oracle(bins, iters):
    hp, mk = batch()
    got = summary(_run_batch(hp, mk, "study", n_bins=bins, max_iters=iters), len(iters))
    assert any(sum(i) > len(iters) for i in got[1])   # the E map ran at more than one slope
    assert_same(got, sweep(bins, iters), range(NB), ("study", bins))
    assert_oracle(got, hp, mk, range(NB), bins, iters, ("study", bins))


@pytest.mark.parametrize("bins,iters", CASES, ids=IDS)
def test_grid_form_equals_sweeps_and_oracle(bins, iters):
    hp, mk = batch()
    got = summary(_run_batch(hp[:1], mk[:1], "grid", n_bins=bins, max_iters=iters), len(iters))
    assert_same(got, sweep(bins, iters), [0], ("grid", bins))
    assert_oracle(got, hp, mk, [0], bins, iters, ("grid", bins))


def test_empty_mask_in_the_batch_leaves_the_others():
    """A study with an empty mask returns before the iteration loop (none of the E map's barriers);
    the other 15 studies compute what they compute without it."""
    hp, mk = batch()
    mk = mk.copy()
    mk[5] = 0
    bins, iters = CASES[0]
    out = _run_batch(hp, mk, "study", n_bins=bins, max_iters=iters)
    got = summary(out, len(iters))
    assert out[4][5].n_mask == 0 and out[1][5].sum() == 0
    assert np.array_equal(got[0][5], hp[5])
    others = [b for b in range(NB) if b != 5]
    assert_same(got, sweep(bins, iters), others, "empty")
    assert_oracle(got, hp, mk, others, bins, iters, "empty")
