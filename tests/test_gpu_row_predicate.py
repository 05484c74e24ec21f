"""The row walks' lane predicate (n4_shared.h item_off: the row's 64-bit mask, ANDed with "the row is
inside the span", is the predicate every select and every dropped store of init and of the two fits
takes; eval forms the same predicate from lane counts and a compare) on masks whose rows are the
predicate's edge cases, through the three drivers and both convergence modes, against the C oracle
and, for conv_mode 0, driver against driver bit for bit.

A tile is 64 consecutive columns of the flattened (C, Z) plane and a row of a tile is one 64-bit
mask.  pattern_mask gives every tile, in an order that shifts from tile to tile, rows with only lane
0, only the tile's last live lane, all lanes, the even lanes, the odd lanes, a single voxel in the
middle and no voxel; row 0 and row R - 1 (the slot's first and last rows: R < 64, one slot) are
non-empty in every tile but the two special ones: one tile holds two rows only (a span shorter than
a group of FIT_G = 6 rows whatever the level: the rows past it run with the predicate off) and one
is empty.  C * Z is no multiple of 64 at the three shapes, so the last tile has dead lanes.  At the
finer levels the control spans are shorter than a group at every shape (37 rows over 8 spans at the
last level, 12 rows over 8)."""
import functools

import numpy as np
import pytest

import n4_param_cases as P
from test_gpu_n4_params import assert_oracle, assert_same, summary
from test_gpu_parity import _run_batch, _run_one

pytestmark = pytest.mark.gpu

DRIVERS = ("study", "grid", "sweep")
SHAPES = ("37x45x7", "24x20x6", "12x70x9")
KINDS = ("lane0", "last", "all", "even", "odd", "single", "none")


def row_bits(kind, live):
    r = np.zeros(64, np.uint8)
    if kind == "lane0":
        r[0] = 1
    elif kind == "last":
        r[live - 1] = 1
    elif kind == "all":
        r[:live] = 1
    elif kind == "even":
        r[0:live:2] = 1
    elif kind == "odd":
        r[1:live:2] = 1
    elif kind == "single":
        r[live // 2] = 1
    return r


def pattern_mask(R, C, Z):
    CZ = C * Z
    nt = (CZ + 63) // 64
    m = np.zeros((R, nt * 64), np.uint8)
    for t in range(nt):
        live = min(64, CZ - 64 * t)
        if nt > 2 and t == 1:     # two rows only, in the middle of the slot
            m[R // 2, 64 * t:64 * t + 64] = row_bits("all", live)
            m[R // 2 + 1, 64 * t:64 * t + 64] = row_bits("odd", live)
            continue
        if nt > 3 and t == nt - 2:   # an empty tile
            continue
        for x in range(R):
            kind = KINDS[(x + 2 * t) % len(KINDS)]
            if x in (0, R - 1) and kind == "none":
                kind = "last" if x == 0 else "lane0"
            m[x, 64 * t:64 * t + 64] = row_bits(kind, live)
    return np.ascontiguousarray(m[:, :CZ]).reshape(R, C, Z)


@functools.lru_cache(maxsize=None)
def case(shape):
    R, C, Z, _ = P.SHAPES[shape]
    X, _ = P.volume(shape)
    M = pattern_mask(R, C, Z)
    M.setflags(write=False)
    return X, M


@functools.lru_cache(maxsize=None)
def ref(shape, conv_mode):
    from oracle import native
    X, M = case(shape)
    return native.n4(X, M, conv_mode=conv_mode)


@functools.lru_cache(maxsize=None)
def gpu(shape, driver, conv_mode):
    X, M = case(shape)
    return summary(_run_one(X, M, driver, conv_mode=conv_mode), 4)


def test_the_masks_hold_the_rows_they_are_built_for():
    for shape in SHAPES:
        R, C, Z, _ = P.SHAPES[shape]
        CZ = C * Z
        assert CZ % 64 != 0
        m = np.asarray(case(shape)[1]).reshape(R, CZ)
        nt = (CZ + 63) // 64
        full = 0
        for t in range(nt):
            rows = m[:, 64 * t:64 * t + 64]
            live = rows.shape[1]
            cnt = rows.sum(axis=1)
            if not cnt.any() or (cnt > 0).sum() == 2:
                continue
            full += 1
            assert cnt[0] > 0 and cnt[-1] > 0
            assert (cnt == live).any() and (cnt == 0).any()
            one = rows[cnt == 1]
            assert one[:, 0].any() and one[:, live - 1].any() and one[:, live // 2].any()
            assert any((r[0:live:2] == 1).all() and not r[1:live:2].any() for r in rows)
        assert full >= 2


@pytest.mark.parametrize("conv_mode", [0, 1])
@pytest.mark.parametrize("driver", DRIVERS)
@pytest.mark.parametrize("shape", SHAPES)
def test_pattern_rows_vs_oracle(shape, driver, conv_mode):
    s = gpu(shape, driver, conv_mode)
    assert sum(s[4]) > 4, s[4]   # the levels iterate: the fit and eval walks run
    assert_oracle(s, ref(shape, conv_mode), conv_mode, (shape, driver))


@pytest.mark.parametrize("shape", SHAPES)
def test_pattern_rows_drivers_agree_bit_for_bit(shape):
    s = gpu(shape, "sweep", 0)
    for driver in ("study", "grid"):
        assert_same(gpu(shape, driver, 0), s, (shape, driver))


@pytest.mark.parametrize("conv_mode", [0, 1])
@pytest.mark.parametrize("driver", DRIVERS)
def test_pattern_study_beside_an_empty_and_a_tiny_one(driver, conv_mode):
    """One batch: the pattern study, a study with an empty mask and one of three voxels.  Every store
    of the empty study is dropped (it comes back as it went in, no iteration), the tiny one equals
    the oracle, and the pattern study equals its run alone bit for bit."""
    from oracle import native
    shape = "37x45x7"
    X, M = case(shape)
    mk = np.zeros((3,) + M.shape, np.uint8)
    mk[0] = M
    mk[2, 17, 20:23, 3] = 1
    hp = np.stack([X, X * np.float32(1.25), X])
    out = _run_batch(hp, mk, driver, conv_mode=conv_mode)
    s = summary(out, 4, 0)
    assert_oracle(s, ref(shape, conv_mode), conv_mode, (driver, "pattern"))
    assert_same(s, gpu(shape, driver, conv_mode), (driver, "pattern alone"))
    assert out[4][1].n_mask == 0 and np.array_equal(out[0][1], hp[1]) and not out[1][1].any()
    assert list(out[4][1].n4_iters[:4]) == [0, 0, 0, 0]
    assert out[4][2].n_mask == 3
    assert_oracle(summary(out, 4, 2), native.n4(hp[2], mk[2], conv_mode=conv_mode), conv_mode, (driver, "tiny"))
