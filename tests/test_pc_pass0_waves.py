"""PC pass 0 by waves (n4_shared.h pcw_run): every wave transposes its own 64 blocks through a tile
of its own and runs as many 8-step groups as its own blocks need, with one workgroup barrier after
the loop.  The masked counts below are the smallest at which that indexing can go wrong (1024
blocks, 64 per wave, groups of 8 steps); both drivers that reach pcw_run (k_n4_study, and the sweep
driver's k_n4_pcw) against the C oracle: iteration counts and convergence values equal, the field
within assert_n4_matches' bound.  (Every case fits the study driver's LDS layout: a ValueError
about the LDS budget at this shape is a failure, not a skip.)"""
import functools

import numpy as np
import pytest

from test_gpu_parity import _run_batch, assert_n4_matches
from oracle import native
from vent_analysis_amd.synth import synth_batch

pytestmark = pytest.mark.gpu

SHAPE = (32, 32, 20)
# the strict interior of the volume holds 30 x 30 x 18 = 16200 voxels; the largest count needs the
# box to reach the last slice as well
BOX = (slice(1, 31), slice(1, 31), slice(1, 19))
BOX_BIG = (slice(1, 31), slice(1, 31), slice(1, 20))

COUNTS = [
    2, 3,                     # smallest non-empty studies: one wave works, 15 have no block
    63, 64, 65,               # last lane of wave 0 / first block of wave 1
    1023, 1024, 1025,         # L 0 -> 1, rem 1023 / 0 / 1: mixed lengths inside and across waves
    8 * 1024 + 5,             # lengths 9 and 8: a partial second group in wave 0 only
    9 * 1024 - 1,             # every wave but the last lane at length 9
    16 * 1024 + 64 * 3 + 1,   # the remainder ends inside wave 3
]


def first_n_mask(n):
    """The first n voxels, in raster order, of the interior box."""
    box = BOX if n <= 30 * 30 * 18 else BOX_BIG
    inner = np.zeros(tuple(s.stop - s.start for s in box), np.uint8)
    assert n <= inner.size
    inner.reshape(-1)[:n] = 1
    m = np.zeros(SHAPE, np.uint8)
    m[box] = inner
    assert int(m.sum()) == n
    return m


@functools.lru_cache(maxsize=None)
def _images():
    hp, _ = synth_batch(*SHAPE, 2, base_seed=60)
    hp.setflags(write=False)
    return hp


@functools.lru_cache(maxsize=None)
def _ref(n, b):
    """The oracle's N4 of image b under the n-voxel mask (computed once, shared by the drivers)."""
    ref, its, conv = native.n4(_images()[b], first_n_mask(n))
    ref.setflags(write=False)
    return ref, its, conv


@pytest.mark.parametrize("driver", ["study", "sweep"])
@pytest.mark.parametrize("n", COUNTS)
def test_pass0_block_counts_vs_oracle(n, driver):
    hp = _images()
    mk = np.stack([first_n_mask(n)] * 2)
    n4, _, _, _, res = _run_batch(hp, mk, driver)
    for b in range(2):
        assert res[b].n_mask == n
        ref, its, conv = _ref(n, b)
        assert_n4_matches(n4[b], res[b].n4_iters[:4], res[b].n4_conv[:4], ref, its, conv, 0,
                          (n, driver, b))


@pytest.mark.parametrize("driver", ["study", "sweep"])
def test_pass0_empty_study_beside_it(driver):
    """n == 0 issues no load at all (the clamped index 0 of an empty study is not a valid rank):
    an all-zero mask beside the 1025-voxel study.  The empty study has no masked voxel and no
    defect voxel, and its N4 output is its input (bias field zero: I / exp(0))."""
    n = 1025
    hp = _images()
    mk = np.stack([first_n_mask(n), np.zeros(SHAPE, np.uint8)])
    n4, d, _, _, res = _run_batch(hp, mk, driver)
    ref, its, conv = _ref(n, 0)
    assert_n4_matches(n4[0], res[0].n4_iters[:4], res[0].n4_conv[:4], ref, its, conv, 0,
                      (n, driver, "beside empty"))
    assert res[1].n_mask == 0 and d[1].sum() == 0
    assert np.array_equal(n4[1], hp[1])
