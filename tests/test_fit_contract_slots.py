"""The S5 fit's contraction of finished control rows (n4_shared.h fit_contract): stage 1 runs only
the live ones of a lane's four output slots (nq = ceil(nr ny KT / 64), a scalar branch per count)
and reads a group of slice steps ahead of its fmas; stage 2 reads a group of cols ahead.  The
shapes below are the smallest at which the contraction changes path; every driver that reaches
fit_contract (k_n4_study in place, the sweep driver's k_n4_fit_items into a separate buffer, the
grid form k_n4_studyg) runs them against the C oracle: iteration counts and convergence values
equal, the field within assert_n4_matches' bound.  Two different studies per launch, so two
workgroups hold rings at different tiles.  (Every case fits the study driver's LDS layout: a
ValueError about the LDS budget at these shapes is a failure, not a skip.)

The paths of a shape follow from the level tables (4, 5, 7, 11 control points per axis) and the
study layout: a tile of 64 (y, z) columns spans ny cols and KT = bz[last] + 4 - bz[first] slice
control points; a ring row takes s_cap = max(64, max ny KT) doubles, the ring nb_ring = min(4,
256 / s_cap) rows (one value per study), a batch nbmax = min(nb_ring, 256 / (ny KT)) rows.
test_shapes_reach_every_contraction_path restates those tables (vh_axis_tables, study_layout,
fit_ring_begin) and asserts what each shape is here for:

| shape     | seeds  | tiles | ny     | nbmax | nq of a full batch, by level | here for                  |
|-----------|--------|-------|--------|-------|------------------------------|---------------------------|
| 64x64x24  | 31, 32 | 24    | 3, 4   | 4     | 1 / 1, 2 / 2 / 3             | the bench's geometry      |
| 40x40x4   | 32, 33 | 3     | 8, 16  | 1     | 1 / 1, 2 / 1, 2 / 2, 3       | a contraction per row     |
| 24x130x3  | 34, 35 | 7     | 2, 22  | 1     | 1, 2 / 1, 2 / 1, 3 / 1, 4    | ny = 22: six col groups   |
| 33x48x12  | 36, 37 | 9     | 6      | 3     | 2 / 2 / 2 / 4                | final batch of one row    |
| 24x20x7   | 38, 39 | 3     | 2, 10  | 2     | 1, 2 / 1, 2 / 1, 3 / 1, 4    | nbmax 2                   |
| 16x5x12   | 40, 41 | 1     | 5      | 4     | 2 / 2 / 3 / 4                | a one-tile study          |

The ring's row count is one value per study (from the largest ny KT of any level), so 40x40x4 and
24x130x3 run every level with nbmax 1 (not 4, 3, 2, 1 and 2, 2, 1, 1 by level); 24x20x7 and
16x5x12 were added for nbmax 2 and the one-tile study.  A level-0 item pushes exactly four rows
(one control span), so nbmax 3 leaves a final contraction of one row and nbmax 4 none.  Tiles
begin and end inside a col (z0 != 0, z1 != Z - 1) at 64x64x24, 24x130x3, 33x48x12 and 24x20x7."""
import functools

import numpy as np
import pytest

from test_gpu_parity import _run_batch, assert_n4_matches
from oracle import native
from vent_analysis_amd.synth import synth_batch

# (shape, base seed): the batch holds the studies of seeds base and base + 1
CASES = [((64, 64, 24), 31), ((40, 40, 4), 32), ((24, 130, 3), 34), ((33, 48, 12), 36),
         ((24, 20, 7), 38), ((16, 5, 12), 40)]
NCP = (4, 5, 7, 11)   # control points per axis by level
TILE_W, FIT_SO, FIT_NB, ST_WAVES = 64, 4, 4, 16


def _base(n, ncp):
    """Control span of every index of an axis (n4.hip vh_axis_tables, float32 steps)."""
    f = np.float32
    spans = ncp - 3
    eps = f(100.0) * np.finfo(f).eps
    while f(NCP[-1] - 3) == f(NCP[-1] - 3) - eps:
        eps = eps * f(10.0)
    scale = f(spans) / f(n - 1)
    out = []
    for i in range(n):
        p = f(i) * scale
        if abs(p - f(spans)) <= eps:
            p = f(spans) - eps
        out.append(int(max(p, f(0.0))))
    return out


def contraction_paths(shape):
    """Per level the (ny, KT, z0, z1) of every tile, and the study's ring rows (study_layout)."""
    _, C, Z = shape
    CZ = C * Z
    levels = []
    for ncp in NCP:
        bz = _base(Z, ncp)
        tiles = []
        for c0 in range(0, CZ, TILE_W):
            c1 = min(c0 + TILE_W, CZ) - 1
            y0, y1, z0, z1 = c0 // Z, c1 // Z, c0 % Z, c1 % Z
            klo = bz[z0 if y0 == y1 else 0]
            KT = bz[z1 if y0 == y1 else Z - 1] + 4 - klo
            tiles.append((y1 - y0 + 1, KT, z0, z1))
        levels.append(tiles)
    s_cap = max(ny * KT for t in levels for ny, KT, _, _ in t)
    assert s_cap <= 64 * FIT_SO, "no LDS geometry for the study driver"
    nb_ring = max(1, min(FIT_NB, 32768 // (ST_WAVES * 8 * max(s_cap, 64))))
    return levels, nb_ring


def _nbmax(nb_ring, ny, KT):
    return max(1, min(nb_ring, 64 * FIT_SO // (ny * KT)))


def _nq(nr, ny, KT):
    return -(-nr * ny * KT // 64)


def test_shapes_reach_every_contraction_path():
    """The table of the module docstring, from the restated level tables (runs without a GPU)."""
    want = {   # shape: (tiles, ny values, nbmax, nq of a full batch by level)
        (64, 64, 24): (24, {3, 4}, 4, [{1}, {1, 2}, {2}, {3}]),
        (40, 40, 4): (3, {8, 16}, 1, [{1}, {1, 2}, {1, 2}, {2, 3}]),
        (24, 130, 3): (7, {2, 22}, 1, [{1, 2}, {1, 2}, {1, 3}, {1, 4}]),
        (33, 48, 12): (9, {6}, 3, [{2}, {2}, {2}, {4}]),
        (24, 20, 7): (3, {2, 10}, 2, [{1, 2}, {1, 2}, {1, 3}, {1, 4}]),
        (16, 5, 12): (1, {5}, 4, [{2}, {2}, {3}, {4}]),
    }
    assert set(want) == {s for s, _ in CASES}
    nq_seen, nb_seen, mid = set(), set(), 0
    for shape, (ntiles, nys, nbmax, nq_by_level) in want.items():
        levels, nb_ring = contraction_paths(shape)
        Z = shape[2]
        assert len(levels[0]) == ntiles and {t[0] for t in levels[0]} == nys, shape
        for L, tiles in enumerate(levels):
            assert {_nbmax(nb_ring, ny, KT) for ny, KT, _, _ in tiles} == {nbmax}, (shape, L)
            nq = {_nq(nbmax, ny, KT) for ny, KT, _, _ in tiles}
            assert nq == nq_by_level[L], (shape, L, nq)
            nq_seen |= nq
        nb_seen.add(nbmax)
        mid += any(z0 != 0 and z1 != Z - 1 for _, _, z0, z1 in levels[0])
    assert nq_seen == {1, 2, 3, 4} and nb_seen == {1, 2, 3, 4} and mid >= 4
    # a final contraction with fewer rows than a full batch, and a smaller live-slot count in it:
    # level 0 pushes four rows per item, so nbmax 3 leaves one row (nq 2 -> 1 at 33x48x12)
    levels, nb_ring = contraction_paths((33, 48, 12))
    ny, KT = levels[0][0][:2]
    assert 4 % _nbmax(nb_ring, ny, KT) == 1 and _nq(1, ny, KT) == 1 and _nq(3, ny, KT) == 2


@functools.lru_cache(maxsize=None)
def _batch(case):
    shape, seed = CASES[case]
    hp, mk = synth_batch(*shape, 2, base_seed=seed)
    hp.setflags(write=False)
    mk.setflags(write=False)
    return hp, mk


@functools.lru_cache(maxsize=None)
def _ref(case, b, conv_mode):
    """The oracle's N4 of study b of a case (computed once, shared by the drivers)."""
    hp, mk = _batch(case)
    ref, its, conv = native.n4(hp[b], mk[b], conv_mode=conv_mode)
    ref.setflags(write=False)
    return ref, its, conv


@pytest.mark.gpu
@pytest.mark.parametrize("conv_mode", [0, 1])
@pytest.mark.parametrize("driver", ["study", "sweep", "grid"])
@pytest.mark.parametrize("case", range(len(CASES)), ids=["x".join(map(str, s)) for s, _ in CASES])
def test_contraction_paths_vs_oracle(case, driver, conv_mode):
    hp, mk = _batch(case)
    n4, _, _, _, res = _run_batch(hp, mk, driver, conv_mode=conv_mode)
    for b in range(2):
        ref, its, conv = _ref(case, b, conv_mode)
        assert min(its) >= 2, (CASES[case], b, list(its))   # every level contracts more than once
        assert_n4_matches(n4[b], res[b].n4_iters[:4], res[b].n4_conv[:4], ref, its, conv, conv_mode,
                          (CASES[case], driver, b))
