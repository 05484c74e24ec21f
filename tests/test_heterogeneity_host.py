"""CPU: the heterogeneity calls exist at every layer (header, library, ctypes) and refuse bad arguments
without touching a device, and the numpy reference the GPU tests compare against (heterogeneity_ref)
equals an independently written per-voxel loop bit for bit, has the known answers a coefficient of
variation must have, and is exercised by inputs that reach all three classes of the summary."""
import ctypes as ct
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO
from vent_analysis_amd import _lib

import heterogeneity_ref as H

F32 = np.float32
NEW = ("vh_batch_heterogeneity", "vh_batch_download_heterogeneity", "vh_heterogeneity")
NAMES = ("mask_stats;gather;sort;mean;classify;cohort;kmeans;snr;border;n4_init;n4_den;n4_hist;"
         "n4_fit;n4_contract;n4_eval;n4_welford;n4_pcw;n4_pcg;n4_final;n4_study;ci_walk;vdp_chain;"
         "ci_walk_b;defect_sel")


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def test_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(REPO, "include", "vent_hip.h")).read()
    L = _lib.lib()
    for n in NEW:
        assert re.search(r"^int %s\(vh_(batch|ctx) \*" % n, hdr, re.M), n
        assert hasattr(L, n), n
        assert n in _lib._SIGS, n
    assert L.vh_batch_kernel_names().decode() == NAMES   # "het_b" is timed but not listed
    assert L.vh_abi_version() == 8   # additions only
    for n in ("heterogeneity", "download_heterogeneity"):
        assert callable(getattr(_lib.Batch, n)), n
    assert callable(_lib.heterogeneity) and callable(_lib.het_index)
    from vent_analysis_amd import Vent_Analysis
    assert callable(Vent_Analysis.ventilation_heterogeneity)
    assert "sets nothing on the object" in Vent_Analysis.ventilation_heterogeneity.__doc__


def test_null_arguments_are_argument_errors():
    """Checked before anything is dereferenced: no device is needed."""
    L = _lib.lib()
    buf = np.ones(64, np.float32)
    p = _lib._ptr(buf)
    assert L.vh_batch_heterogeneity(None, 1, 5, 64, ct.c_float(0.5), 0) == _lib.VH_ERR_ARG
    assert L.vh_batch_download_heterogeneity(None, p, p, p) == _lib.VH_ERR_ARG
    assert L.vh_heterogeneity(None, p, p, 2, 2, 2, 1, 1, 5, 64, ct.c_float(0.5), p, p, p) == _lib.VH_ERR_ARG


@pytest.mark.parametrize("kw", [dict(radius=0), dict(radius=6), dict(radius=1.0), dict(radius=True),
                                dict(min_count=1), dict(min_count=10), dict(radius=2, min_count=26),
                                dict(min_count=2.0), dict(bins=0), dict(bins=1025), dict(bins=64.0),
                                dict(hi=0.0), dict(hi=-1.0), dict(hi=np.inf), dict(hi=np.nan), dict(hi=16.5)],
                         ids=str)
def test_argument_errors_are_value_errors(kw):
    """The checks of vh_batch_heterogeneity, made by the binding first (so the message names the
    argument): ValueError, and no device is touched."""
    a = dict(radius=1, min_count=None, bins=100, hi=1.0)
    a.update(kw)
    with pytest.raises(ValueError):
        _lib._heterogeneity_args(a["radius"], a["min_count"], a["bins"], a["hi"])


def test_argument_defaults_and_forms():
    assert _lib._heterogeneity_args(1, None, 100, 1.0) == (1, 5, 100, 1.0)       # a majority of 9
    assert _lib._heterogeneity_args(2, None, 1, 16) == (2, 13, 1, 16.0)
    assert _lib._heterogeneity_args(5, None, 1024, 0.5) == (5, 61, 1024, 0.5)
    assert _lib._heterogeneity_args(np.int64(3), np.int32(49), np.int64(7), F32(0.25)) == (3, 49, 7, 0.25)
    assert _lib._heterogeneity_args(1, 2, 64, 0.1)[3] == float(F32(0.1))         # hi as the float32 the library gets
    assert _lib._heterogeneity_args(1, 9, 64, 1.0)[1] == 9


def test_het_index():
    st = np.array([[4, 1, 2, 3 << 24], [0, 5, 0, 0], [3, 0, 0, (1 << 24) + 1]], np.int64)
    got = _lib.het_index(st)
    assert got.dtype == np.float64 and got.shape == (3,)
    assert got[0] == 0.75 and np.isnan(got[1]) and got[2] == ((1 << 24) + 1) / 16777216.0 / 3.0
    assert _lib.het_index(st[0]) == 0.75


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_batch_state_row_under_sanitizers(tmp_path):
    """tests/heterogeneity_state_check.cpp, a stand-alone program over the header the library includes:
    the guard, the transition (nothing else changes) and what discards the result."""
    csrc = os.path.join(REPO, "vent_analysis_amd", "csrc")
    exe = str(tmp_path / "chk")
    subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", csrc, os.path.join(REPO, "tests", "heterogeneity_state_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "heterogeneity state ok" in r.stdout, r.stdout + r.stderr


# ---- the reference itself ------------------------------------------------------------------------
def brute(x, M, radius, min_count):
    """The spec read voxel by voxel, every operation on np.float32 scalars."""
    R, C, Z = x.shape
    k = radius
    out = np.zeros(x.shape, F32)
    with np.errstate(all="ignore"):
        for z in range(Z):
            for r in range(R):
                for c in range(C):
                    if not M[r, c, z]:
                        continue
                    nb = [x[r + dr, c + dc, z] for dr in range(-k, k + 1) for dc in range(-k, k + 1)
                          if 0 <= r + dr < R and 0 <= c + dc < C and M[r + dr, c + dc, z]]
                    n = len(nb)
                    s = F32(0)
                    for v in nb:
                        s = F32(s + v)
                    m = F32(s / F32(n))
                    q = F32(0)
                    for v in nb:
                        t = F32(v - m)
                        q = F32(q + F32(t * t))
                    if n >= min_count and m > 0:
                        out[r, c, z] = F32(np.sqrt(F32(q / F32(n - 1))) / m)
                    else:
                        out[r, c, z] = F32(-1)
    return out


@pytest.mark.parametrize("radius,min_count", H.PARAMS)
def test_reference_equals_a_per_voxel_loop(radius, min_count):
    """Bit for bit, on (5, 7, 3) and a 12 x 11 x 2 crop of the (41, 37, 9) inputs that straddles the
    zeroed ellipse and the mask's rim, both studies with a mask."""
    x, mk = H.batch_inputs((5, 7, 3)), H.batch_masks((5, 7, 3)) != 0
    for q in range(2):
        assert np.array_equal(bits(H.cov_map(x[q], mk[q], radius, min_count)), bits(brute(x[q], mk[q], radius, min_count)))
    x, mk = H.batch_inputs((41, 37, 9)), H.batch_masks((41, 37, 9)) != 0
    crop = (slice(6, 18), slice(8, 19), slice(3, 5))
    for q in range(2):
        xc, mc = np.ascontiguousarray(x[q][crop]), np.ascontiguousarray(mk[q][crop])
        assert mc.any() and not mc.all()
        got, ref = H.cov_map(xc, mc, radius, min_count), brute(xc, mc, radius, min_count)
        assert np.array_equal(bits(got), bits(ref)), (q, int((bits(got) != bits(ref)).sum()))


@pytest.mark.parametrize("radius,min_count", H.PARAMS)
def test_known_answers(radius, min_count):
    shape = (41, 37, 9)
    x, mk = H.batch_inputs(shape)[0], H.batch_masks(shape)[0] != 0
    out = H.cov_map(x, mk, radius, min_count)
    # outside the mask +0 (the bits, not the value); inside never +0 ... unless cv is 0, which this field never gives
    assert not bits(out)[~mk].any() and (out[mk] != 0).all()
    # a constant field: cv == 0 wherever there is a value (the sum of n equal floats up to 121 is exact)
    const = H.cov_map(np.full(shape, 3.0, F32), mk, radius, min_count)
    assert set(np.unique(const[mk]).tolist()) <= {-1.0, 0.0} and (const[mk] == 0).any()
    assert np.array_equal(const == -1, out == -1)          # a value or none: the mask's geometry alone here
    # a power of two scales every sum, mean and difference exactly: the same bits
    assert np.array_equal(bits(H.cov_map(x * F32(4), mk, radius, min_count)), bits(out))
    # fewer than min_count mask neighbours: -1 (an isolated voxel has n == 1)
    lone = np.zeros(shape, bool)
    lone[20, 18, 4] = True
    lone[0, 0, 0] = lone[0, 1, 0] = True
    o = H.cov_map(x, lone, radius, min_count)
    assert o[20, 18, 4] == -1
    assert (o[0, 0, 0] == -1) == (min_count > 2) and np.count_nonzero(o) == 3


@pytest.mark.parametrize("radius,min_count", H.PARAMS)
@pytest.mark.parametrize("shape", H.SHAPES, ids=str)
def test_summary_adds_up_and_the_index_is_the_mean(shape, radius, min_count):
    mk = H.batch_masks(shape) != 0
    maps, hist, stats = H.batch_reference(shape, radius, min_count)
    assert hist.dtype == np.uint32 and stats.dtype == np.int64 and hist.shape == (3, H.BINS)
    assert not np.isnan(maps).any()
    for q in range(3):
        assert stats[q, :3].sum() == mk[q].sum()
        assert hist[q].sum() == stats[q, 0]
        v = maps[q][mk[q]]
        inside = v[(v >= 0) & (v < F32(H.HI))]
        assert inside.size == stats[q, 0] and (v == -1).sum() == stats[q, 2]
        if inside.size:   # every term is truncated by less than 2^-24
            mean = inside.astype(np.float64).mean()
            idx = _lib.het_index(stats[q])
            assert idx == H.index(stats[q]) and abs(mean - idx) < 2.0 ** -24, (mean, idx)
        else:
            assert np.isnan(_lib.het_index(stats[q]))
    assert not stats[2].any() and not hist[2].any() and not bits(maps[2]).any()   # the empty mask


def test_inputs_exercise_all_three_classes():
    """At every shape but the smallest: voxels inside [0, hi) and voxels at or above it under every
    parameter set, voxels without a value under at least two of the three, and at least 36 of the 64
    bins occupied by the first study."""
    for shape in H.SHAPES[1:]:
        none = 0
        for radius, min_count in H.PARAMS:
            _, hist, stats = H.batch_reference(shape, radius, min_count)
            assert stats[:, 0].any() and stats[:, 1].any(), (shape, radius, stats)
            none += bool(stats[:, 2].any())
            assert 36 <= np.count_nonzero(hist[0]) <= 64, (shape, radius, np.count_nonzero(hist[0]))
        assert none >= 2, shape
    small = H.batch_reference(H.SHAPES[0], 2, 13)[2]
    assert small[0, 0] and small[0, 2] and small[1, 2]      # a slice smaller than the window still has both
