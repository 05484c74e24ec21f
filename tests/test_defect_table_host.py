"""CPU: the defect-table calls exist at every layer (header, library, ctypes, class) and refuse bad
arguments without touching a device; the reference the GPU tests compare against (defect_table_ref)
agrees with hand-made cases whose answers are known and with a plain loop over the voxels;
table_metrics gives the hand values; and the state row holds under sanitizers."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO
from vent_analysis_amd import _lib

import components_ref as K
import defect_table_ref as T

NEW = ("vh_batch_defect_table", "vh_batch_download_defect_table")
NAMES = ("mask_stats;gather;sort;mean;classify;cohort;kmeans;snr;border;n4_init;n4_den;n4_hist;"
         "n4_fit;n4_contract;n4_eval;n4_welford;n4_pcw;n4_pcg;n4_final;n4_study;ci_walk;vdp_chain;"
         "ci_walk_b;defect_sel")


def test_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(REPO, "include", "vent_hip.h")).read()
    L = _lib.lib()
    for n in NEW:
        assert re.search(r"^int %s\(vh_batch \*" % n, hdr, re.M), n
        assert hasattr(L, n), n
        assert n in _lib._SIGS, n
    assert re.search(r"^#define VH_DT_COLS 18$", hdr, re.M) and re.search(r"^#define VH_DT_MAX_ROWS 1024$", hdr, re.M)
    assert re.search(r"^#define VH_DT_NO_SIGNAL \(-1\)$", hdr, re.M)
    assert (_lib.VH_DT_COLS, _lib.VH_DT_MAX_ROWS, _lib.VH_DT_NO_SIGNAL) == (18, 1024, -1)
    assert len(_lib.DT_COLUMNS) == 18 == T.COLS and _lib.DT_COLUMNS[T.FACES_Z] == "faces_z"
    assert L.vh_batch_kernel_names().decode() == NAMES              # "dtab_b" is timed but not listed
    assert L.vh_abi_version() == 8                                  # additions only
    for n in ("defect_table", "download_defect_table"):
        assert callable(getattr(_lib.Batch, n)), n
    assert callable(_lib.table_metrics)
    from vent_analysis_amd import Vent_Analysis
    assert callable(Vent_Analysis.defect_table)
    assert "sets nothing on the object" in Vent_Analysis.defect_table.__doc__


def test_null_handles_are_argument_errors():
    """Checked before anything is dereferenced: no device is needed."""
    L = _lib.lib()
    buf = np.ones(64, np.uint32)
    p = _lib._ptr(buf)
    for norm in (-1, 0, 1):
        assert L.vh_batch_defect_table(None, p, 64, norm) == _lib.VH_ERR_ARG
    assert L.vh_batch_download_defect_table(None, p, p) == _lib.VH_ERR_ARG
    assert L.vh_batch_download_defect_table(None, None, None) == _lib.VH_ERR_ARG


def test_argument_helper():
    h = _lib._defect_table_args
    ms, n, norm = h(1, 64, None, 3)
    assert ms.dtype == np.uint32 and ms.tolist() == [1, 1, 1] and (n, norm) == (64, -1)
    ms, n, norm = h([5, 1, 2 ** 32 - 1], 1024, "p99", 3)
    assert ms.tolist() == [5, 1, 2 ** 32 - 1] and (n, norm) == (1024, 1)
    assert h(np.int64(7), np.int32(1), "mean", 2)[1:] == (1, 0) and type(h(1, np.int32(9), None, 1)[1]) is int
    for bad in (0, -1, [1, 0, 1], [1, 1], 1.0, True, 2 ** 32, [[1, 1, 1]], None, "1"):
        with pytest.raises(ValueError):
            h(bad, 64, None, 3)
    for bad in (0, 1025, -5, 64.0, True, None, "64", (64,)):
        with pytest.raises(ValueError):
            h(1, bad, None, 3)
    for bad in ("median", "MEAN", 0, 1, -1, True, 0.0, ("mean",)):
        with pytest.raises(ValueError):
            h(1, 64, bad, 3)


def test_class_refuses_before_calculate_vdp():
    from vent_analysis_amd import Vent_Analysis
    va = Vent_Analysis.__new__(Vent_Analysis)                # (the constructor computes the mask's border on the GPU)
    va.device, va.defectArray, va.N4HPvent, va.vox = 0, '', '', [1.5, 1.5, 10.0]
    va.mask = np.ones((4, 4, 2))
    before = dict(vars(va))
    with pytest.raises(ValueError, match="not set"):
        va.defect_table()
    va.N4HPvent = np.ones((4, 4, 2), np.float32)
    with pytest.raises(ValueError, match="not set"):
        va.defect_table()
    va.N4HPvent = ''
    assert set(vars(va)) == set(before) and all(vars(va)[k] is before[k] for k in before)
    va.N4HPvent, va.defectArray = np.ones((4, 4, 2), np.float32), np.ones((4, 4, 2))
    for kw in (dict(conn=7), dict(min_size=0), dict(max_rows=0), dict(max_rows=1025), dict(norm="median"),
               dict(max_rows=2.0), dict(min_size=True)):
        with pytest.raises(ValueError):                      # the helpers, before any device
            va.defect_table(**kw)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_batch_state_row_under_sanitizers(tmp_path):
    """tests/defect_table_state_check.cpp, a stand-alone program over the header the library includes:
    enqueue, need, and the discards by a new labelling, by the filter and by a run."""
    csrc = os.path.join(REPO, "vent_analysis_amd", "csrc")
    exe = str(tmp_path / "chk")
    subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", csrc, os.path.join(REPO, "tests", "defect_table_state_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "defect table state ok" in r.stdout, r.stdout + r.stderr


def test_design_names_the_state_row():
    txt = open(os.path.join(REPO, "DESIGN.md")).read()
    assert "defect_table_enqueued" in txt and "need_defect_table()" in txt


# ---- the reference against the known ---------------------------------------------------------------
def one_table(a, conn, min_size=1, max_rows=8, x=None, d=None):
    root, _, roots, sizes = K.components(a, conn)
    return T.table(root, roots, sizes, min_size, max_rows, x, d)


def test_a_cube():
    """2 x 2 x 2 inside 4 x 4 x 4 at (1..2)^3: size 8, sums 12, bounds 1..2, 8 faces per axis."""
    a = np.zeros((4, 4, 4), np.uint8)
    a[1:3, 1:3, 1:3] = 1
    for conn in (6, 26):
        rows, stats = one_table(a, conn)
        assert rows[0].tolist() == [(1 * 4 + 1) * 4 + 1, 8, 12, 12, 12, 1, 2, 1, 2, 1, 2, 8, 8, 8, 0, 0, 0, 0]
        assert (rows[1:, 0] == -1).all() and not rows[1:, 1:].any() and stats.tolist() == [1, 1, 8, 8]
    rows, stats = one_table(a, 4)                            # per slice: two 2 x 2 squares, the lower slice first
    assert stats.tolist() == [2, 2, 8, 8]
    assert rows[0].tolist() == [21, 4, 6, 6, 4, 1, 2, 1, 2, 1, 1, 4, 4, 8, 0, 0, 0, 0]
    assert rows[1].tolist() == [22, 4, 6, 6, 8, 1, 2, 1, 2, 2, 2, 4, 4, 8, 0, 0, 0, 0]
    rows, stats = one_table(a, 6, min_size=9)                # nothing qualifies: zero rows
    assert stats.tolist() == [0, 0, 0, 0] and (rows[:, 0] == -1).all() and not rows[:, 1:].any()


def test_a_plus():
    """A plus of 5 voxels in one slice at the volume's edge (its top arm on row 0): 12 in-plane faces,
    2 per voxel across the slice."""
    a = np.zeros((5, 5, 1), np.uint8)
    a[1, 1:4, 0] = 1
    a[0:3, 2, 0] = 1
    rows, stats = one_table(a, 4)
    assert rows[0].tolist() == [2, 5, 5, 10, 0, 0, 2, 1, 3, 0, 0, 6, 6, 10, 0, 0, 0, 0] and stats.tolist() == [1, 1, 5, 5]
    x = np.full(a.shape, 0.5, np.float32)
    x[1, 1, 0], x[1, 3, 0], x[0, 2, 0] = np.nan, -1.0, 200.0       # three of the five are not counted
    x[0, 0, 0] = 1.0                                               # off the component: never read
    rows, _ = one_table(a, 4, x=x, d=2.0)
    assert rows[0, T.N_SIG:].tolist() == [2, 2 * 2 ** 22, 2 ** 22, 2 ** 22]
    rows, _ = one_table(a, 4, x=np.full(a.shape, -0.0, np.float32), d=2.0)
    assert rows[0, T.N_SIG:].tolist() == [5, 0, 0, 0]              # -0 counts, as 0
    for d in (0.0, np.inf, np.nan):
        xx = x if d == 0.0 else np.full(a.shape, np.inf, np.float32)
        assert one_table(a, 4, x=xx, d=d)[0][0, T.N_SIG:].tolist() == [0, 0, 0, 0]
    rows, _ = one_table(a, 4, x=np.full(a.shape, 63.999996, np.float32), d=1.0)
    assert rows[0, T.N_SIG:].tolist() == [5, 5 * (2 ** 30 - 64), 2 ** 30 - 64, 2 ** 30 - 64]
    rows, _ = one_table(a, 4, x=np.full(a.shape, 64.0, np.float32), d=1.0)
    assert rows[0, T.N_SIG:].tolist() == [0, 0, 0, 0]


def test_the_smaller_root_ranks_first():
    """Two bars of 3 voxels and one of 2: the bars in the order of their roots, then the short one;
    max_rows cuts the rank order, min_size its tail."""
    a = np.zeros((7, 4, 1), np.uint8)
    a[0, :2, 0] = 1
    a[2, 1:, 0] = 2
    a[5, :3, 0] = 3
    rows, stats = one_table(a, 4, max_rows=4)
    assert rows[:, 0].tolist() == [9, 20, 0, -1] and rows[:, 1].tolist() == [3, 3, 2, 0]
    assert stats.tolist() == [3, 3, 8, 8]
    rows, stats = one_table(a, 4, max_rows=1)
    assert rows[:, 0].tolist() == [9] and stats.tolist() == [1, 3, 3, 8]
    rows, stats = one_table(a, 4, min_size=3, max_rows=2)
    assert rows[:, 0].tolist() == [9, 20] and stats.tolist() == [2, 2, 6, 6]
    out = T.reference(np.stack([a, a]), 4, (3, 1), 2)
    assert out["stats"].tolist() == [[2, 2, 6, 6], [2, 3, 6, 8]] and out["truncated"].tolist() == [False, True]


@pytest.mark.parametrize("conn", K.CONNS)
@pytest.mark.parametrize("shape", [(5, 3, 1), (41, 37, 9)], ids=str)
def test_the_reference_is_a_loop_over_the_voxels(shape, conn):
    a = K.batch_inputs(shape)
    for q in (K.FULL, K.RAND40, K.BRIDGE, K.DIAGONAL) if shape[0] > 5 else range(K.N_STUDIES):
        root, _, roots, sizes = K.components(a[q], conn)
        broot, bsize = K.bfs_components(a[q], conn)
        for ms, n in ((1, 5), (2, 64)):
            rows, stats = T.table(root, roots, sizes, ms, n)
            brows, bstats = T.brute_force(broot, bsize, ms, n)
            assert np.array_equal(rows, brows) and np.array_equal(stats, bstats), (q, ms, n)
            if conn in (4, 8):
                assert np.array_equal(rows[:, T.FACES_Z], 2 * rows[:, T.SIZE])   # slices never join


# ---- table_metrics ---------------------------------------------------------------------------------
def test_table_metrics():
    vox = (1.5, 2.0, 10.0)
    rows = np.zeros((2, 3, 18), np.int64)
    rows[:, :, 0] = -1
    rows[0, 0] = [21, 8, 12, 12, 12, 1, 2, 1, 2, 1, 2, 8, 8, 8, 4, 3 * 2 ** 24, 2 ** 23, 2 ** 24]
    rows[0, 1] = [5, 1, 0, 1, 2, 0, 0, 1, 1, 2, 2, 2, 2, 2, 0, 0, 0, 0]
    m = _lib.table_metrics(rows, vox)
    assert all(v.dtype == np.float64 for v in m.values())
    assert m["volume_mL"].shape == (2, 3) and m["centroid"].shape == (2, 3, 3) and m["extent"].shape == (2, 3, 3)
    assert m["volume_mL"][0, 0] == 8 * (0.15 * 0.2 * 1.0) and m["volume_mL"][0, 1] == 0.15 * 0.2 * 1.0
    assert m["centroid"][0, 0].tolist() == [1.5, 1.5, 1.5] and m["centroid_mm"][0, 0].tolist() == [2.25, 3.0, 15.0]
    assert m["centroid"][0, 1].tolist() == [0.0, 1.0, 2.0]
    assert m["extent"][0, 0].tolist() == [2.0, 2.0, 2.0] and m["extent"][0, 1].tolist() == [1.0, 1.0, 1.0]
    s0 = 8 * 2.0 * 10.0 + 8 * 1.5 * 10.0 + 8 * 1.5 * 2.0
    assert m["surface_mm2"][0, 0] == s0 and m["surface_mm2"][0, 1] == s0 / 4
    assert abs(m["sphericity"][0, 0] / (np.pi ** (1 / 3) * (6 * 8 * 30.0) ** (2 / 3) / s0) - 1) < 1e-14   # (two pow calls)
    assert (m["mean"][0, 0], m["min"][0, 0], m["max"][0, 0]) == (0.75, 0.5, 1.0)
    for k in ("mean", "min", "max"):
        assert np.isnan(m[k][0, 1])                                  # n_sig = 0
    for k, v in m.items():
        assert np.isnan(v[0, 2]).all() and np.isnan(v[1]).all(), k   # unused rows
    cube = _lib.table_metrics(rows[0, 0], (1.0, 1.0, 1.0))           # one row; a cube of side 2: pi/6 of its sphere
    assert cube["volume_mL"].shape == () and abs(cube["sphericity"] - (np.pi / 6) ** (1 / 3)) < 1e-14
    with pytest.raises(ValueError):
        _lib.table_metrics(rows[..., :17], vox)
    with pytest.raises(ValueError):
        _lib.table_metrics(rows, (1.0, 1.0))
