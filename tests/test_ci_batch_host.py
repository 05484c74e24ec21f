"""CPU: the batch cluster-index calls exist at every layer (header, library, ctypes), refuse null
arguments without touching a device, and ci_expand rebuilds the oracle's float64 map from shells."""
import ctypes as ct
import os
import re

import numpy as np
import pytest

from conftest import REPO
from oracle import native
from vent_analysis_amd import _lib
from vent_analysis_amd.sphere import compact_table_for

NEW = ("vh_batch_ci", "vh_batch_set_defect", "vh_batch_download_ci")
VOX = (1.5, 1.5, 10.0)


def test_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(REPO, "include", "vent_hip.h")).read()
    L = _lib.lib()
    for n in NEW:
        assert re.search(r"^int %s\(vh_batch \*b" % n, hdr, re.M), n
        assert hasattr(L, n), n
        assert n in _lib._SIGS, n
    assert "ci_walk_b" in L.vh_batch_kernel_names().decode().split(";")
    assert L.vh_abi_version() == 8   # additions only


def test_null_batch_is_an_argument_error():
    """Checked before anything is dereferenced: no device is needed."""
    L = _lib.lib()
    buf = np.zeros(8, np.uint8)
    assert L.vh_batch_ci(None, None, ct.c_double(1.5)) == _lib.VH_ERR_ARG
    assert L.vh_batch_ci(None, _lib._ptr(buf), ct.c_double(1.5)) == _lib.VH_ERR_ARG
    assert L.vh_batch_set_defect(None, _lib._ptr(buf)) == _lib.VH_ERR_ARG
    assert L.vh_batch_download_ci(None, None, None, _lib._ptr(buf), _lib._ptr(buf)) == _lib.VH_ERR_ARG


def _blobs(shape, seed):
    rng = np.random.default_rng(seed)
    i, j, k = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    d = np.zeros(shape, bool)
    for _ in range(7):
        c = [rng.uniform(-0.1, 1.1) * s for s in shape]
        r = rng.uniform(3, 12)
        d |= (i - c[0]) ** 2 + (j - c[1]) ** 2 + ((k - c[2]) * 3) ** 2 <= r * r
    d &= rng.random(shape) > 0.15
    return d


def _four_voxels(shape):
    d = np.zeros(int(np.prod(shape)), np.uint8)
    d[np.random.default_rng(8).choice(d.size, 4, replace=False)] = 1
    return d.reshape(shape)


@pytest.mark.parametrize("d,Rmax", [
    (np.random.default_rng(7).random((41, 37, 9)) < 0.2, 12),
    (_four_voxels((41, 37, 9)), 12),
    (_blobs((70, 90, 12), 1), 50),
], ids=["random-0.2", "four-voxels", "blobs-70x90x12"])
def test_ci_expand_equals_the_oracle_map(d, Rmax):
    table = compact_table_for(VOX, Rmax, d.shape)
    ref, shell = native.ci(d, table, VOX)
    got = _lib.ci_expand(shell.astype(np.int16), table.radii, min(VOX))
    assert got.dtype == np.float64 and got.shape == ref.shape
    assert np.array_equal(got, ref)
    assert np.array_equal(_lib.ci_expand(shell, table.radii, min(VOX)), ref)   # any integer dtype


def test_ci_expand_refuses_bad_shells():
    radii = np.array([0.5, 1.0, 1.5])
    ok = _lib.ci_expand(np.array([-1, 0, 2], np.int16), radii, 2.0)
    assert np.array_equal(ok, [0.0, 1.0, 3.0])
    with pytest.raises(ValueError):
        _lib.ci_expand(np.array([0.0, 1.0]), radii, 2.0)          # not an integer dtype
    with pytest.raises(ValueError):
        _lib.ci_expand(np.array([0, 1], bool), radii, 2.0)
    with pytest.raises(ValueError):
        _lib.ci_expand(np.array([0, 3], np.int16), radii, 2.0)    # shell == len(radii)
    assert _lib.ci_expand(np.zeros((0,), np.int16), radii, 2.0).shape == (0,)
