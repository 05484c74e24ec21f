"""The S3 histogram of the volume-resident kernels (n4_study.hip hist_slice: 16 compact values per
thread and trip, one packed 64-bit LDS add per value into one of the histogram copies, the copies
summed by the E map) against the C oracle.

Masked-voxel counts of 1, 15, 16, 17, 16 * 1024 - 1 and 16 * 1024 + 5 at 37, 200 and 256 bins: a
thread without a value, the tail path of a thread's 16 (one value short, full, one over), a whole
workgroup trip but one value, and a second trip of five.  The mask is a run of consecutive voxels
of a 64x64x8 volume, which gives the count exactly.  A mask of one voxel has no fit (n < 2): the
study comes back as it went in.  One study has a constant intensity inside the mask, so in the
first histogram every lane of every add hits the same bin (the worst collision, and the largest
count one copy's word holds: 16 389 < 2^20), one has two intensities at the ends of the range.
Every level runs to its cap (the threshold is far below what two iterations reach), so a run
builds nine histograms.  The last case is the largest lattice the kernels accept (ncp (4, 6, 4):
11x27x11): it must run on `study` and `grid`, not be refused for LDS."""
import functools

import numpy as np
import pytest

import n4_param_cases as P
from test_gpu_n4_params import assert_oracle, assert_same, summary
from test_gpu_parity import _run_one
from vent_analysis_amd.synth import synth_volume

pytestmark = pytest.mark.gpu

SHAPE = (64, 64, 8)
START = 64 * 8 * 9 + 3      # the run's first voxel: inside a row, no multiple of 16
COUNTS = (15, 16, 17, 16 * 1024 - 1, 16 * 1024 + 5)
BINS = (37, 200, 256)
CAPS = (3, 2, 2, 2)
DRIVERS = ("study", "grid")


def kw(bins):
    return dict(n_bins=bins, max_iters=CAPS, conv_threshold=1e-7)


def run_mask(count):
    m = np.zeros(SHAPE[0] * SHAPE[1] * SHAPE[2], np.uint8)
    m[START:START + count] = 1
    return m.reshape(SHAPE)


@functools.lru_cache(maxsize=None)
def case(kind):
    """kind: a count (the synthetic image) or 'const' / 'two' (the largest count)."""
    X, _ = synth_volume(*SHAPE, 21)
    M = run_mask(kind if isinstance(kind, int) else COUNTS[-1])
    if kind == "const":
        X = X.copy()
        X[M == 1] = 100.0
    elif kind == "two":
        X = X.copy()
        v, idx = X.reshape(-1), np.flatnonzero(M.reshape(-1))
        v[idx[0::2]] = 10.0
        v[idx[1::2]] = 1000.0
    X.setflags(write=False)
    M.setflags(write=False)
    return X, M


@functools.lru_cache(maxsize=None)
def ref(kind, bins):
    from oracle import native
    X, M = case(kind)
    return native.n4(X, M, **kw(bins))


@functools.lru_cache(maxsize=None)
def gpu(kind, bins, driver):
    X, M = case(kind)
    return summary(_run_one(X, M, driver, **kw(bins)), 4)


@pytest.mark.parametrize("driver", DRIVERS)
@pytest.mark.parametrize("bins", BINS)
@pytest.mark.parametrize("kind", COUNTS + ("const", "two"))
def test_histogram_counts_vs_oracle(kind, bins, driver):
    assert int(case(kind)[1].sum()) == (kind if isinstance(kind, int) else COUNTS[-1])
    r = ref(kind, bins)
    if kind != "two":   # (two intensities: the field difference is zero and a level ends at once)
        assert list(r[1])[1:] == list(CAPS)[1:], r[1]
    assert_oracle(gpu(kind, bins, driver), r, 0, (kind, bins, driver))


@pytest.mark.parametrize("bins", BINS)
@pytest.mark.parametrize("kind", COUNTS + ("const", "two"))
def test_histogram_drivers_agree_bit_for_bit(kind, bins):
    assert_same(gpu(kind, bins, "grid"), gpu(kind, bins, "study"), (kind, bins))


@pytest.mark.parametrize("driver", DRIVERS)
def test_one_masked_voxel_has_no_histogram(driver):
    X, _ = synth_volume(*SHAPE, 21)
    out = _run_one(X, run_mask(1), driver, **kw(200))
    assert out[4][0].n_mask == 1 and np.array_equal(out[0][0], X)
    assert list(out[4][0].n4_iters[:4]) == [0, 0, 0, 0]


@pytest.mark.parametrize("driver", DRIVERS)
def test_largest_accepted_lattice_still_runs(driver):
    """ncp (4, 6, 4) with four levels, 11x27x11 control points at the last: no "LDS budget" refusal
    (an exception fails the test), and the oracle's result."""
    shape, c = "37x45x7", "ncp-y"
    assert P.params(c) == dict(ncp=(4, 6, 4))
    X, M = P.volume(shape)
    s = summary(_run_one(X, M, driver, **P.params(c)), 4)
    assert_oracle(s, P.oracle(shape, c), 0, (shape, c, driver))
