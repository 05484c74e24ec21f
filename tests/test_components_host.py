"""CPU: the connected-components calls exist at every layer (header, library, ctypes, class) and refuse
bad arguments without touching a device; the reference the GPU tests compare against (components_ref:
scipy.ndimage.label, bincount, minimum.at, the rank rule) agrees with a plain breadth-first search over
the definition's offsets and with hand-made cases whose answers are known; and the shared inputs are
not trivial."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO
from vent_analysis_amd import _lib

import components_ref as K

NEW = ("vh_batch_components", "vh_batch_download_components", "vh_batch_filter_components", "vh_components",
       "vh_filter_components")
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
    assert re.search(r"^#define VH_CC_DEFECT 0$", hdr, re.M) and re.search(r"^#define VH_CC_MASK 1$", hdr, re.M)
    assert (_lib.VH_CC_DEFECT, _lib.VH_CC_MASK) == (0, 1)
    assert "count is NOT updated" in hdr                             # the header says what download_defect's count is
    assert "connectivity across slices, component size filters" not in hdr   # the "not done" list points to the calls
    assert L.vh_batch_kernel_names().decode() == NAMES              # "comp_b" is timed but not listed
    assert L.vh_abi_version() == 8                                  # additions only
    for n in ("components", "download_components", "filter_components"):
        assert callable(getattr(_lib.Batch, n)), n
    assert callable(_lib.components) and callable(_lib.filter_components)
    from vent_analysis_amd import Vent_Analysis
    for n in ("defect_components", "filter_defects", "clean_mask"):
        assert callable(getattr(Vent_Analysis, n)), n
    assert "sets nothing on the object" in Vent_Analysis.defect_components.__doc__


def test_null_arguments_are_argument_errors():
    """Checked before anything is dereferenced: no device is needed."""
    L = _lib.lib()
    buf = np.ones(64, np.uint32)
    p = _lib._ptr(buf)
    assert L.vh_batch_components(None, 0, 6, p, 1) == _lib.VH_ERR_ARG
    assert L.vh_batch_download_components(None, p, p, p, p) == _lib.VH_ERR_ARG
    assert L.vh_batch_filter_components(None, 0, 6, p, None, None) == _lib.VH_ERR_ARG
    assert L.vh_components(None, p, 2, 2, 2, 1, 6, p, 0, p, p, p, p) == _lib.VH_ERR_ARG
    assert L.vh_filter_components(None, p, 2, 2, 2, 1, 6, p, None, p, p) == _lib.VH_ERR_ARG


def test_components_argument_helper():
    h = _lib._components_args
    s, c, e = h("defect", 6, ())
    assert (s, c) == (0, 6) and e.dtype == np.uint32 and e.shape == (0,)
    assert h("mask", 26, (2, 5))[:2] == (1, 26) and h(1, 4, [2])[2].tolist() == [2]
    assert h(0, 8, np.arange(2, 33))[2].tolist() == list(range(2, 33))       # 31 edges
    assert h("mask", 6, (2, 2 ** 32 - 1))[2].tolist() == [2, 2 ** 32 - 1]
    for bad in (5, 0, 18, 6.0, "6", True, None):
        with pytest.raises(ValueError):
            h("defect", bad, ())
    for bad in ("lungs", 2, -1, None, 0.0):
        with pytest.raises(ValueError):
            h(bad, 6, ())
    for bad in ((1,), (0, 2), (2, 2), (5, 3), (2, 2 ** 32), (-3,), tuple(range(2, 34)), (2.0, 3.0), (True,),
                ((2, 3),)):
        with pytest.raises(ValueError):
            h("defect", 6, bad)


def test_filter_argument_helper():
    h = _lib._filter_components_args
    s, c, ms, kl = h("mask", 6, 1, 0, 3)
    assert (s, c) == (1, 6) and ms.dtype == np.uint32 and ms.tolist() == [1, 1, 1]
    assert kl.dtype == np.int32 and kl.tolist() == [0, 0, 0]
    s, c, ms, kl = h("defect", 8, [5, 1, 2 ** 32 - 1], (8, 0, 2), 3)
    assert ms.tolist() == [5, 1, 2 ** 32 - 1] and kl.tolist() == [8, 0, 2]
    for ms, kl in ((0, 0), (-1, 0), ([1, 0, 1], 0), (1, 9), (1, -1), (1, [0, 0, 9]), ([1, 1], 0), (1, [1, 1]),
                   (1.0, 0), (1, 2.0), (True, 0), (2 ** 32, 0), ([[1, 1, 1]], 0)):
        with pytest.raises(ValueError):
            h("defect", 6, ms, kl, 3)
    with pytest.raises(ValueError):
        h("defect", 7, 1, 0, 3)
    with pytest.raises(ValueError):
        h("both", 6, 1, 0, 3)


def test_the_bindings_check_before_any_device():
    """ValueError from the argument helpers, before a context is made."""
    a = np.ones((4, 4, 2), np.uint8)
    with pytest.raises(ValueError):
        _lib.components(a, conn=5)
    with pytest.raises(ValueError):
        _lib.components(a, edges=(1,))
    with pytest.raises(ValueError):
        _lib.filter_components(a, min_size=0)
    with pytest.raises(ValueError):
        _lib.filter_components(a, keep_largest=9)


def test_class_refusals():
    from vent_analysis_amd import Vent_Analysis
    va = Vent_Analysis.__new__(Vent_Analysis)                # (the constructor computes the mask's border on the GPU)
    va.device, va.defectArray, va.vox = 0, '', [1.5, 1.5, 10.0]
    va.mask = np.ones((4, 4, 2))
    with pytest.raises(ValueError, match="not set"):
        va.defect_components()
    with pytest.raises(ValueError, match="not set"):
        va.filter_defects(3)
    va.defectArray = np.ones((4, 4, 2))
    with pytest.raises(ValueError):
        va.defect_components(conn=7)
    with pytest.raises(ValueError):
        va.defect_components(edges=(5, 3))
    with pytest.raises(ValueError):
        va.filter_defects(0)
    with pytest.raises(ValueError):
        va.clean_mask(keep_largest=9)
    with pytest.raises(ValueError):
        va.clean_mask(min_size=0)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_batch_state_row_under_sanitizers(tmp_path):
    """tests/components_state_check.cpp, a stand-alone program over the header the library includes:
    the guard, the transition (nothing else changes), what keeps the result and what discards it."""
    csrc = os.path.join(REPO, "vent_analysis_amd", "csrc")
    exe = str(tmp_path / "chk")
    subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", csrc, os.path.join(REPO, "tests", "components_state_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "components state ok" in r.stdout, r.stdout + r.stderr


# ---- the reference itself ------------------------------------------------------------------------
@pytest.mark.parametrize("conn", K.CONNS)
@pytest.mark.parametrize("shape", [(2, 2, 1), (5, 3, 1), (9, 11, 4), (8, 8, 30)], ids=str)
def test_the_reference_is_a_breadth_first_search(shape, conn):
    """scipy's labels with bincount and minimum.at against a plain search over the definition's
    offsets, on every shared study."""
    ref = K.batch_reference(shape, conn)
    for q, a in enumerate(K.batch_inputs(shape)):
        root, size = K.bfs_components(a, conn)
        assert np.array_equal(ref["root"][q], root), (q, conn)
        assert np.array_equal(ref["size"][q], size), (q, conn)
    assert ref["root"].dtype == np.int32 and ref["size"].dtype == np.uint32
    assert ref["counts"].dtype == np.int64 and ref["stats"].dtype == np.int64 and ref["stats"].shape == (K.N_STUDIES, 4)


def test_the_checkerboard():
    """V / 2 components of size 1 at 4 neighbours, one component at 8; with one slice 6 is 4 and 26 is 8."""
    R, C = 6, 8
    a = K.batch_inputs((R, C, 1))[K.CHECKER]
    for conn, n in ((4, R * C // 2), (6, R * C // 2), (8, 1), (26, 1)):
        root, size, roots, sizes = K.components(a, conn)
        assert len(roots) == n and sizes.sum() == R * C // 2, conn
        if n > 1:
            assert (sizes == 1).all() and np.array_equal(root[a != 0], np.flatnonzero(a.ravel()))
        else:
            assert roots[0] == 0 and (root[a != 0] == 0).all() and (size[a != 0] == R * C // 2).all()
        assert (root[a == 0] == -1).all() and (size[a == 0] == 0).all()
    a3 = K.batch_inputs((R, C, 3))[K.CHECKER]                     # three slices: columns of 3 along Z at 6 neighbours
    assert (K.components(a3, 6)[3] == 3).all() and len(K.components(a3, 4)[2]) == 3 * R * C // 2


def test_a_corner_contact_across_slices():
    """Two voxels that touch only by a corner across slices: one component at 26, two at 6, 4 and 8."""
    a = np.zeros((3, 3, 2), np.uint8)
    a[0, 0, 0] = a[1, 1, 1] = 1
    for conn, n in ((26, 1), (6, 2), (4, 2), (8, 2)):
        root, size, roots, sizes = K.components(a, conn)
        assert len(roots) == n, conn
    root = K.components(a, 26)[0]
    assert root[0, 0, 0] == 0 and root[1, 1, 1] == 0
    assert K.components(a, 6)[0][1, 1, 1] == (1 * 3 + 1) * 2 + 1


def test_ties_go_to_the_smaller_root():
    """Three bars of 3 voxels and one of 2: the largest is the first bar; keep_largest = 2 keeps the first
    two; the ranks follow (size, -root)."""
    a = np.zeros((7, 4, 1), np.uint8)
    a[0, :3, 0] = 1
    a[2, :2, 0] = 2
    a[4, 1:, 0] = 3
    a[6, :3, 0] = 4
    root, size, roots, sizes = K.components(a, 4)
    assert roots.tolist() == [0, 8, 17, 24] and sizes.tolist() == [3, 2, 3, 3]
    counts, stats = K.summary(roots, sizes, (3,))
    assert stats.tolist() == [11, 4, 3, 0] and counts.tolist() == [[1, 2], [3, 9]]
    assert K.ranks(roots, sizes).tolist() == [0, 3, 1, 2]
    out, nc, nv = K.filter_volume(a, 4, 1, 2)
    assert (nc, nv) == (2, 6) and np.array_equal(out != 0, (a == 1) | (a == 3)) and set(np.unique(out)) == {0, 1, 3}
    out, nc, nv = K.filter_volume(a, 4, 3, 0)
    assert (nc, nv) == (3, 9) and np.array_equal(out != 0, (a != 0) & (a != 2)) and out.dtype == a.dtype
    out, nc, nv = K.filter_volume(a, 4, 3, 8)                     # more than there are: min_size alone decides
    assert (nc, nv) == (3, 9)
    out, nc, nv = K.filter_volume(a, 4, 1, 4)
    assert (nc, nv) == (4, 11) and np.array_equal(out, a)
    out, nc, nv = K.filter_volume(a, 4, 4, 1)                     # the rank counts every component: nothing passes both
    assert (nc, nv) == (0, 0) and not out.any()
    e = K.summary(np.zeros(0, np.int64), np.zeros(0, np.int64), (2, 5))
    assert e[1].tolist() == [0, 0, 0, -1] and not e[0].any() and e[0].shape == (3, 2)


@pytest.mark.parametrize("shape", K.SHAPES[2:], ids=str)
def test_the_shared_inputs_are_not_trivial(shape):
    """Many components in the random studies, components that span several tiles, parts that join only
    through another slice or only by a diagonal step, and the two extremes."""
    a = K.batch_inputs(shape)
    V = int(np.prod(shape))
    plane_tiles = -(-shape[0] // K.TILE[0]) * -(-shape[1] // K.TILE[1])
    tiles = plane_tiles * -(-shape[2] // K.TILE[2])
    for conn in K.CONNS:
        ref = K.batch_reference(shape, conn, K.EDGE_SETS[2])
        st = ref["stats"]
        assert st[K.EMPTY].tolist() == [0, 0, 0, -1] and not ref["size"][K.EMPTY].any()
        assert (ref["root"][K.EMPTY] == -1).all()
        assert st[K.FULL, 0] == V and st[K.FULL, 3] == 0
        assert st[K.FULL, 1] == (1 if conn in (6, 26) else shape[2])
        if conn != 26:   # (26 neighbours at these densities: far above percolation, one component is likely)
            assert (st[[K.RAND40, K.RAND60], 1] > 1).all()
        else:
            assert st[K.DIAGONAL, 1] > 1 and (st[[K.RAND40, K.RAND60], 1] >= 1).all()
        assert np.array_equal(ref["counts"][:, :, 0].sum(axis=1), st[:, 1])
        assert np.array_equal(ref["counts"][:, :, 1].sum(axis=1), st[:, 0])
        for q in (K.RAND60, K.SERPENTINE):
            if (tiles if conn in (6, 26) else plane_tiles) > 1:
                assert K.tiles_spanned(ref["root"][q], st[q, 3]) > 1, (conn, q)
        assert K.tiles_spanned(ref["root"][K.SERPENTINE], st[K.SERPENTINE, 3]) == (tiles if conn in (6, 26) else plane_tiles)
        assert st[K.SERPENTINE, 1] == (1 if conn in (6, 26) else shape[2])
        if shape[2] > 1 and shape[0] > 2:
            assert st[K.BRIDGE, 1] == (1 if conn in (6, 26) else 3)
        n_diag = st[K.DIAGONAL, 1]
        if conn in (4, 6):
            assert n_diag == st[K.DIAGONAL, 0]                   # no diagonal link: every voxel on its own
        elif conn == 8:
            assert n_diag < st[K.DIAGONAL, 0]                    # the in-plane lines hold; the one along Z does not
        else:
            assert 2 <= n_diag <= 4                              # the three lines and the lone voxel
    assert (a[K.RAND40] == 255).any() and (a[K.RAND40] == 2).any()
