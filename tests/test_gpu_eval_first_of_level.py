"""Eval of a level's first iteration (n4_study.hip eval_item<false, CM>): the previous field's T
windows were written with the previous level's tables, so the old window and the new one move at
different rows.  The loop walks spans that end at the next boundary of either window, in prefetched
row groups like every other iteration, with the previous level's row tables staged in LDS.

Both drivers that share eval_pass run here against the C oracle with the comparison of the other N4
parity tests (assert_n4_matches: iteration counts and convergence values equal, the output within
one ulp): k_n4_study on a batch of 16 studies, the grid form k_n4_studyg on one.  Every study runs
at least two iterations in levels 1 and 2 (test_cases_iterate_in_levels_1_and_2, without a GPU),
so the first-of-level loop and the loop that follows it both run in those levels.

Row span starts by level (4, 5, 7, 11 control points) and what a shape is here for:

| case      | span starts, levels 1 / 2 / 3                          | here for                              |
|-----------|--------------------------------------------------------|---------------------------------------|
| 24x16x4   | 12 / 6.. by 6 / 3.. by 3                               | one row slot; spans of 3 rows (half a |
|           |                                                        | group) ending on new-only and on      |
|           |                                                        | shared boundaries in one item         |
| 37x20x3   | 18 / 9, 18, 27 / 5, 9, 14, 18, 23, 27, 32              | odd R, uneven spans (4 and 5 rows),   |
|           |                                                        | a last span shorter than a group      |
| 128x16x2  | 64 / 32, 64, 96 / 16.. by 16                           | two row slots: spans of more than two |
|           |                                                        | groups, items that begin inside a     |
|           |                                                        | span of both levels                   |
| 70x12x5   | 35 / 18, 35, 52 / 9, 18, 26, 35, 44, 52, 61            | two row slots: the slot boundary (64) |
|           |                                                        | falls between an old-level boundary   |
|           |                                                        | (52) and a new-only one (61)          |
| column    | (37x20x3)                                              | masks of one voxel column: 63 lanes   |
|           |                                                        | of every group masked out             |
| two-iters | (24x16x4) conv_threshold 0, two iterations per level   | the first-of-level eval followed by   |
|           |                                                        | exactly one other                     |
"""
import functools

import numpy as np
import pytest

from test_gpu_parity import _run_batch, assert_n4_matches
from oracle import native
from vent_analysis_amd.synth import synth_volume

NB = 16   # studies of a k_n4_study launch
SEEDS = list(range(100, 116))
# name: (shape, seeds, column masks, N4 options); a seed is left out where the oracle runs a single
# iteration in level 1 or 2 (test_cases_iterate_in_levels_1_and_2)
CASES = {
    "24x16x4": ((24, 16, 4), SEEDS, False, {}),
    "37x20x3": ((37, 20, 3), SEEDS, False, {}),
    "128x16x2": ((128, 16, 2), [s for s in range(100, 117) if s != 111], False, {}),
    "70x12x5": ((70, 12, 5), SEEDS, False, {}),
    "column": ((37, 20, 3), [s for s in range(100, 118) if s not in (108, 116)], True, {}),
    "two-iters": ((24, 16, 4), SEEDS, False, dict(conv_threshold=0.0, max_iters=(2, 2, 2, 2))),
}


@functools.lru_cache(maxsize=None)
def _batch(name):
    shape, seeds, column, _ = CASES[name]
    assert len(seeds) == NB
    hp = np.empty((NB,) + shape, np.float32)
    mk = np.zeros((NB,) + shape, np.uint8)
    for b, s in enumerate(seeds):
        x, m = synth_volume(*shape, s, vary=True)
        hp[b] = x
        if column:   # one (y, z) column of the study's mask: the one with the most voxels
            cnt = m.sum(axis=0)
            y, z = np.unravel_index(int(np.argmax(cnt)), cnt.shape)
            mk[b, :, y, z] = m[:, y, z]
        else:
            mk[b] = m
    hp.setflags(write=False)
    mk.setflags(write=False)
    return hp, mk


@functools.lru_cache(maxsize=None)
def _ref(name, b, conv_mode):
    """The oracle's N4 of study b of a case (computed once, shared by the drivers)."""
    hp, mk = _batch(name)
    ref, its, conv = native.n4(hp[b], mk[b], conv_mode=conv_mode, **CASES[name][3])
    ref.setflags(write=False)
    return ref, its, conv


@pytest.mark.parametrize("conv_mode", [0, 1])
@pytest.mark.parametrize("name", list(CASES))
def test_cases_iterate_in_levels_1_and_2(name, conv_mode):
    """Every study runs the first-of-level eval and another one in levels 1 and 2 (oracle only)."""
    hp, mk = _batch(name)
    for b in range(NB):
        _, its, _ = _ref(name, b, conv_mode)
        assert its[1] >= 2 and its[2] >= 2, (name, b, list(its))
        if name == "column":
            assert (mk[b].sum(axis=0) > 0).sum() == 1 and mk[b].sum() >= 8, (b, int(mk[b].sum()))
        if name == "two-iters":
            assert list(its) == [2, 2, 2, 2], (b, list(its))


@pytest.mark.gpu
@pytest.mark.parametrize("conv_mode", [0, 1])
@pytest.mark.parametrize("name", list(CASES))
def test_study_batch_vs_oracle(name, conv_mode):
    """k_n4_study, 16 studies per launch."""
    hp, mk = _batch(name)
    n4, _, _, _, res = _run_batch(hp, mk, "study", conv_mode=conv_mode, **CASES[name][3])
    for b in range(NB):
        ref, its, conv = _ref(name, b, conv_mode)
        assert_n4_matches(n4[b], res[b].n4_iters[:4], res[b].n4_conv[:4], ref, its, conv, conv_mode,
                          (name, "study", b))


@pytest.mark.gpu
@pytest.mark.parametrize("conv_mode", [0, 1])
@pytest.mark.parametrize("name", list(CASES))
def test_grid_study_vs_oracle(name, conv_mode):
    """k_n4_studyg, one study over several workgroups."""
    hp, mk = _batch(name)
    n4, _, _, _, res = _run_batch(hp[:1], mk[:1], "grid", conv_mode=conv_mode, **CASES[name][3])
    ref, its, conv = _ref(name, 0, conv_mode)
    assert_n4_matches(n4[0], res[0].n4_iters[:4], res[0].n4_conv[:4], ref, its, conv, conv_mode,
                      (name, "grid", 0))
