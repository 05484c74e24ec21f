"""CPU: the denoise calls exist at every layer (header, library, ctypes) and refuse bad arguments
without touching a device, and the numpy reference the GPU tests compare against (denoise_ref) has the
properties a denoise option is wanted for: it leaves a constant alone, its noise estimate finds the
sigma of a magnitude background, and it recovers a phantom."""
import ctypes as ct
import os
import re

import numpy as np
import pytest

from conftest import REPO
from vent_analysis_amd import _lib

import denoise_ref as D

F32 = np.float32
NEW = ("vh_batch_noise_sigma", "vh_batch_denoise", "vh_batch_download_hp", "vh_noise_sigma", "vh_denoise")
NAMES = ("mask_stats;gather;sort;mean;classify;cohort;kmeans;snr;border;n4_init;n4_den;n4_hist;"
         "n4_fit;n4_contract;n4_eval;n4_welford;n4_pcw;n4_pcg;n4_final;n4_study;ci_walk;vdp_chain;"
         "ci_walk_b;defect_sel")


def test_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(REPO, "include", "vent_hip.h")).read()
    L = _lib.lib()
    for n in NEW:
        assert re.search(r"^int %s\(vh_(batch|ctx) \*" % n, hdr, re.M), n
        assert hasattr(L, n), n
        assert n in _lib._SIGS, n
    assert "Vent_Analysis.py:1025" in hdr
    assert L.vh_batch_kernel_names().decode() == NAMES   # "denoise_b" is timed but not listed
    assert L.vh_abi_version() == 8   # additions only
    for n in ("noise_sigma", "denoise", "download_hp"):
        assert callable(getattr(_lib.Batch, n)), n
    assert callable(_lib.noise_sigma) and callable(_lib.denoise)
    from vent_analysis_amd import Vent_Analysis
    assert callable(Vent_Analysis.estimate_noise) and callable(Vent_Analysis.denoise)


def test_null_arguments_are_argument_errors():
    """Checked before anything is dereferenced: no device is needed."""
    L = _lib.lib()
    buf = np.ones(64, np.float32)
    p = _lib._ptr(buf)
    assert L.vh_batch_noise_sigma(None, p) == _lib.VH_ERR_ARG
    assert L.vh_batch_denoise(None, p, ct.c_float(2.0), 3, 1, 0) == _lib.VH_ERR_ARG
    assert L.vh_batch_download_hp(None, p) == _lib.VH_ERR_ARG
    assert L.vh_noise_sigma(None, p, p, 2, 2, 2, 1, p) == _lib.VH_ERR_ARG
    assert L.vh_denoise(None, p, 2, 2, 2, 1, p, ct.c_float(2.0), 3, 1, 0, p) == _lib.VH_ERR_ARG


@pytest.mark.parametrize("kw", [dict(search=0), dict(search=6), dict(patch=-1), dict(patch=3),
                                dict(strength=0.0), dict(strength=-1.0), dict(strength=np.inf),
                                dict(strength=np.nan), dict(sigma=0.0), dict(sigma=-2.0),
                                dict(sigma=np.nan), dict(sigma=np.inf), dict(sigma=[3.0, 0.0]),
                                dict(search=2.5)], ids=str)
def test_argument_errors_are_value_errors(kw):
    """The checks of vh_batch_denoise, made by the binding first (so the message names the argument):
    ValueError, and no device is touched."""
    a = dict(sigma=[3.0, 4.0], n=2, strength=2.0, search=3, patch=1)
    a.update(kw)
    with pytest.raises(ValueError):
        _lib._denoise_args(a["sigma"], a["n"], a["strength"], a["search"], a["patch"])


def test_argument_forms():
    sg, s, p = _lib._denoise_args(3.5, 3, 2.0, np.int64(5), 0)
    assert sg.dtype == F32 and sg.flags.c_contiguous and sg.tolist() == [3.5, 3.5, 3.5] and (s, p) == (5, 0)
    with pytest.raises(ValueError):
        _lib._denoise_args([1.0, 2.0], 3, 2.0, 3, 1)   # two sigmas for three studies


@pytest.mark.parametrize("patch", (0, 1, 2))
@pytest.mark.parametrize("sigma,strength", [(9.5, 2.0), (23.25, 0.7), (1e-3, 2.0), (3e4, 1.3), (1e-30, 1.0)])
def test_host_constants_equal_the_reference(sigma, strength, patch):
    """_lib.denoise_constants is the library's host arithmetic restated: inv_h2 and bias, in double
    from the float32 arguments, rounded once -- the reference's, bit for bit (the last case overflows
    inv_h2 to +inf in both)."""
    a, b = _lib.denoise_constants(sigma, strength, patch), D.constants(sigma, strength, patch)
    assert all(x.dtype == F32 for x in a + b)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    s, k = float(F32(sigma)), float(F32(strength))
    if sigma > 1e-20:
        assert a[0] == F32(1.0 / (2.0 * (2 * patch + 1) ** 2 * (k * s) ** 2)) and a[1] == F32(2.0 * s * s)
    else:
        assert np.isinf(a[0])


# ---- the reference itself ------------------------------------------------------------------------
@pytest.mark.parametrize("search,patch", D.PARAMS)
def test_a_constant_volume_comes_back(search, patch):
    x = np.full((5, 7, 3), 3.0, F32)
    out = D.denoise(x, 1.5, 2.0, search, patch)
    assert out.dtype == F32 and out.tobytes() == x.tobytes()


def test_weights_are_compactly_supported():
    """A pixel whose every other patch is far away keeps its value exactly: all weights but the
    centre's are exact zeros."""
    x = np.full((9, 9, 1), 10.0, F32)
    x[4, 4, 0] = 500.0
    out = D.denoise(x, 1.0, 2.0, 3, 0)
    assert out[4, 4, 0] == F32(500.0)
    out[4, 4, 0] = 10.0
    assert np.all(out == F32(10.0))


@pytest.mark.parametrize("sigma", (10, 25))
def test_phantom_recovery(sigma):
    """The 64 x 64 x 6 phantom (denoise_ref.phantom: two ellipsoids, the generator's bias ramp, one
    radius-4 disc defect at 0.2) under complex Gaussian noise, default_rng(0).  The estimate over the
    complement of the mask lies within 2 % of sigma (measured: 10.007 and 25.017), and at strength
    2.0, (3, 1), rician off, the RMSE to the clean image inside the mask falls below 0.6 of the
    noisy image's (measured with this reference alone: 0.436 and 0.408; with rician on 0.439 and
    0.407)."""
    clean, m = D.phantom()
    x = D.noisy(clean, sigma)
    est = D.sigma_of(x[~m])
    assert est.dtype == F32 and abs(float(est) - sigma) <= 0.02 * sigma, est
    out = D.denoise(x, est, 2.0, 3, 1, False)
    c = clean[m].astype(np.float64)
    rmse = lambda a: float(np.sqrt(np.mean((a[m].astype(np.float64) - c) ** 2)))  # noqa: E731
    print(sigma, float(est), rmse(x), rmse(out), rmse(out) / rmse(x))
    assert rmse(out) < 0.6 * rmse(x), (rmse(out), rmse(x))


def test_noise_sigma_follows_calculate_snrs_noise_box():
    """The estimate reads exactly the voxels oracle.vdp_oracle.noise_mask selects, and is NaN where
    calculate_SNR is undefined: an empty mask, a mask in column 0 only, no row inside the FOV band."""
    from oracle import vdp_oracle as O
    shape = (64, 64, 24)
    hp, mk = D.batch_inputs(shape), D.batch_masks(shape)
    nm = O.noise_mask(mk[0].astype(np.float64))
    v = hp[0][nm].astype(np.float64)
    assert 0 < v.size < hp[0].size
    assert D.noise_sigma(hp[0], mk[0]) == F32(np.sqrt((v * v).sum() / (2.0 * v.size)))
    assert np.isnan(D.noise_sigma(hp[2], mk[2]))
    col0 = np.zeros(shape, np.uint8)
    col0[30:34, 0, :] = 1
    assert np.isnan(D.noise_sigma(hp[0], col0))
    assert np.isnan(D.noise_sigma(D.batch_inputs((5, 7, 3))[0], D.batch_masks((5, 7, 3))[0]))


def test_class_methods_are_documented_as_returning():
    from vent_analysis_amd import Vent_Analysis
    assert "sets nothing on the object" in Vent_Analysis.denoise.__doc__
    assert "sets nothing on the object" in Vent_Analysis.estimate_noise.__doc__
    assert "assign" in Vent_Analysis.denoise.__doc__
