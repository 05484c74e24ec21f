"""CPU: the regional analysis exists at every layer (header, library, ctypes), refuses null handles
without touching a device, its two host functions (vh_zone_parts, vh_zone_split) equal the numpy
reference of the zone rule, the binding helpers raise for every argument the library would refuse,
BatchState's zones row and zones_host.h hold under the sanitizers, and the reference the GPU tests
compare against is itself pinned against the distribution's reference."""
import ctypes as ct
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO
from vent_analysis_amd import _lib

import distribution_ref as DR
import zones_ref as R

NEW = ("vh_batch_zones", "vh_batch_download_zones", "vh_zones", "vh_zone_parts", "vh_zone_split")
NAMES = ("mask_stats;gather;sort;mean;classify;cohort;kmeans;snr;border;n4_init;n4_den;n4_hist;"
         "n4_fit;n4_contract;n4_eval;n4_welford;n4_pcw;n4_pcg;n4_final;n4_study;ci_walk;vdp_chain;"
         "ci_walk_b;defect_sel")
CSRC = os.path.join(REPO, "vent_analysis_amd", "csrc")
BYS = ("extent", "count")


def test_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(REPO, "include", "vent_hip.h")).read()
    L = _lib.lib()
    for n in NEW:
        assert re.search(r"^int %s\((vh_(batch|ctx) \*|const int64_t \*profile)" % n, hdr, re.M), n
        assert hasattr(L, n), n
        assert n in _lib._SIGS, n
    for name, val in (("VH_ZONE_EXTENT", 0), ("VH_ZONE_COUNT", 1), ("VH_ZONE_COLS", 8)):
        assert re.search(r"^#define %s\s+%d\b" % (name, val), hdr, re.M), name
        assert getattr(_lib, name) == val
    assert L.vh_batch_kernel_names().decode() == NAMES   # "zones_b" is timed but not listed
    assert L.vh_abi_version() == 8   # additions only
    for f in ("zones", "zone_by", "zone_parts", "zone_split", "zone_vdp", "zone_mean", "_zones_args"):
        assert callable(getattr(_lib, f)), f
    assert callable(_lib.Batch.zones) and callable(_lib.Batch.download_zones)


def test_null_handles_are_argument_errors():
    """Checked before anything is dereferenced: no device is needed."""
    L = _lib.lib()
    buf = np.zeros(64, np.int64)
    p = _lib._ptr(buf)
    parts = np.array([3, 1, 1], np.int32)
    assert L.vh_batch_zones(None, None, 0, _lib._ptr(parts), 1, 0, 0, 100, ct.c_float(1.5)) == _lib.VH_ERR_ARG
    assert L.vh_batch_download_zones(None, p, p, p, p, p) == _lib.VH_ERR_ARG
    assert L.vh_zones(None, p, p, None, 2, 2, 2, 1, ct.c_float(0.6), None, 0, _lib._ptr(parts), 1, 0, 0, 4,
                      ct.c_float(1.5), p, p, p, p, p) == _lib.VH_ERR_ARG
    part = np.zeros(8, np.uint8)
    b2 = np.zeros(2, np.int32)
    s = ct.c_int32(0)
    ok = (p, 8, 3, 0, _lib._ptr(part), _lib._ptr(b2))
    assert L.vh_zone_parts(*ok) == _lib.VH_OK
    for i, bad in ((0, None), (1, 0), (2, 0), (2, 33), (3, 2), (3, -1), (4, None), (5, None)):
        a = list(ok)
        a[i] = bad
        assert L.vh_zone_parts(*a) == _lib.VH_ERR_ARG, (i, bad)
    assert L.vh_zone_split(p, 8, ct.byref(s)) == _lib.VH_OK
    assert L.vh_zone_split(None, 8, ct.byref(s)) == _lib.VH_ERR_ARG
    assert L.vh_zone_split(p, 0, ct.byref(s)) == _lib.VH_ERR_ARG
    assert L.vh_zone_split(p, 8, None) == _lib.VH_ERR_ARG
    neg = np.array([1, -1, 2], np.int64)
    assert L.vh_zone_parts(_lib._ptr(neg), 3, 2, 0, _lib._ptr(part), _lib._ptr(b2)) == _lib.VH_ERR_ARG
    assert L.vh_zone_split(_lib._ptr(neg), 3, ct.byref(s)) == _lib.VH_ERR_ARG
    with pytest.raises(ValueError):
        _lib.zone_parts(neg, 2)
    with pytest.raises(ValueError):
        _lib.zone_split(neg)


def parts_profiles():
    rng = np.random.default_rng(11)
    big = np.array([0, (1 << 30) - 3, 5, 1 << 29, (1 << 29) - 7, 1, 0, 3], np.int64)   # total just under 2^31
    return {
        "equal": np.full(12, 5, np.int64),
        "single": np.array([0, 0, 0, 9, 0, 0], np.int64),
        "zero": np.zeros(7, np.int64),
        "narrow": np.array([0, 0, 3, 1, 0, 0, 0, 0, 0], np.int64),            # w = 2: p > w for most p
        "heavy": np.array([0, 2, 1, 40, 3, 2, 1, 0, 1], np.int64),            # one plane above half the total
        "holes": np.array([0, 4, 0, 0, 7, 1, 0, 2, 0, 0], np.int64),          # zero planes inside the bounds
        "random": rng.integers(0, 50, 97).astype(np.int64),
        "big": big,
    }


@pytest.mark.parametrize("by", BYS)
@pytest.mark.parametrize("name", list(parts_profiles()))
def test_zone_parts_equals_the_reference(name, by):
    prof = parts_profiles()[name]
    for p in range(1, 33):
        part, (lo, hi) = _lib.zone_parts(prof, p, by)
        assert part.dtype == np.uint8 and (lo, hi) == R.bounds(prof), (p, lo, hi)
        ref = R.axis_parts(prof, p, by)
        assert np.array_equal(part, ref), (p, part, ref)
        assert part.max() <= p - 1 and (np.diff(part.astype(int)) >= 0).all()
    if name == "zero":
        assert (lo, hi) == (0, -1) and not part.any()
    if name == "big":
        assert int(prof.sum()) * 32 > 1 << 35 and prof.sum() < 1 << 31   # a 32-bit product would wrap
    if name == "heavy" and by == "count":
        assert len(set(_lib.zone_parts(prof, 4, by)[0])) < 4              # a part is empty


def test_zone_parts_names_and_ints():
    prof = parts_profiles()["random"]
    assert np.array_equal(_lib.zone_parts(prof, 5, 0)[0], _lib.zone_parts(prof, 5, "extent")[0])
    assert np.array_equal(_lib.zone_parts(prof, 5, 1)[0], _lib.zone_parts(prof, 5, "count")[0])
    assert [_lib.zone_by(b) for b in ("extent", "count", 0, 1, np.int64(1))] == [0, 1, 0, 1, 1]
    for bad in ("Extent", "area", 2, -1, 0.0, None, True):
        with pytest.raises(ValueError):
            _lib.zone_by(bad)
    for bad in (0, 33, -1, 2.0, True):
        with pytest.raises(ValueError):
            _lib.zone_parts(prof, bad)
    with pytest.raises(ValueError):
        _lib.zone_parts(np.zeros((2, 2), np.int64), 2)


SPLITS = {
    "tie": ([5, 1, 7, 0, 0, 0, 6, 1, 5], 3),                 # several zero columns: the smallest wins
    "outside": ([5, 0, 7, 4, 3, 4, 6, 0, 5], 4),             # the zeros lie outside the candidate window
    "edge_lo": ([9, 9, 2, 9, 9, 9, 3, 9, 9], 2),             # the minimum at the window's first column
    "edge_hi": ([9, 9, 3, 9, 9, 9, 2, 9, 9], 6),             # ... and at its last
    "w3": ([0, 3, 2, 3, 0], 2),                              # w_c < 4: the whole interval
    "w2_tie": ([0, 0, 4, 4, 0], 2),
    "w1": ([0, 0, 6, 0], 2),                                 # a single column: s = lo
    "zero": ([0, 0, 0], 0),
    "offset": ([0, 0, 0, 8, 6, 1, 5, 1, 7, 9, 0, 0], 5),     # lo = 3, w = 7, q = 1: candidates 4 .. 8
}


@pytest.mark.parametrize("name", list(SPLITS))
def test_zone_split_equals_the_reference(name):
    prof, want = SPLITS[name]
    assert R.split(prof) == want
    assert _lib.zone_split(prof) == want
    rng = np.random.default_rng(len(name))
    for n in (1, 2, 3, 4, 5, 8, 31, 200):
        p = rng.integers(0, 4, n)
        assert _lib.zone_split(p) == R.split(p), p


def test_argument_errors_of_the_binding():
    """Every error of the library's list, raised by the helper before the library is called."""
    A = _lib._zones_args
    a = A()
    assert (a["K"], a["bins"], a["hi"], a["lateral"], a["by"], a["norm"], list(a["parts"])) == \
        (6, 100, 1.5, 1, 0, 0, [3, 1, 1]) and a["labels"] is None and a["parts"].dtype == np.int32
    assert A(parts=(2, 3, 2), lateral=False)["K"] == 12 and A(parts=(4, 1, 4), lateral=True)["K"] == 32
    assert A(parts=(32, 1, 1), lateral=False, by="count", norm="p99", bins=256, hi=64.0)["K"] == 32
    for bad in (dict(norm=2), dict(norm=-1), dict(norm="median"),
                dict(bins=0), dict(bins=257), dict(bins=-3), dict(bins=10.0),
                dict(hi=0.0), dict(hi=-1.5), dict(hi=float("inf")), dict(hi=float("nan")), dict(hi=64.5),
                dict(by=2), dict(by=-1), dict(by="area"),
                dict(parts=(0, 1, 1)), dict(parts=(3, 1, -1)), dict(parts=(3, 1)), dict(parts=(1.5, 1, 1)),
                dict(parts=(3, 2, 1)),                                # lateral with parts[1] != 1
                dict(parts=(17, 1, 1)), dict(parts=(3, 1, 6)),        # K = 34, 36 with lateral
                dict(parts=(33, 1, 1), lateral=False), dict(parts=(3, 4, 3), lateral=False),
                dict(lateral=2), dict(lateral=-1), dict(lateral=None), dict(lateral="yes")):
        with pytest.raises(ValueError):
            A(**bad)
    lab = np.zeros((1, 4, 4, 2), np.uint8)
    lab[0, 1, 1, 0] = 5
    assert A(labels=lab, shape=lab.shape)["K"] == 5                   # n_zones None: the largest label
    got = A(labels=lab, n_zones=9, parts=(0, 0, 0), lateral=7, by="area", shape=lab.shape)   # geometry not looked at
    assert got["K"] == got["n_zones"] == 9 and got["labels"].dtype == np.uint8
    for bad in (dict(n_zones=0), dict(n_zones=33), dict(n_zones=-1), dict(n_zones=2.0)):
        with pytest.raises(ValueError):
            A(labels=lab, shape=lab.shape, **bad)
    with pytest.raises(ValueError):
        A(labels=np.zeros_like(lab), shape=lab.shape)                 # no label at all: K = 0
    with pytest.raises(ValueError):
        A(labels=lab, shape=(1, 4, 4, 3))
    with pytest.raises(ValueError):
        A(labels=lab.astype(np.float32), shape=lab.shape)
    wide = np.array([[[[300, -2], [3, 0]]]])                          # outside a byte: no zone
    assert A(labels=wide, n_zones=4)["labels"].tolist() == [[[[0, 0], [3, 0]]]]


def test_zone_vdp_and_mean():
    counts = np.zeros((2, 3, 8), np.int64)
    counts[0, 1, :2] = (8, 2)
    counts[1, 2, :2] = (5, 5)
    v = _lib.zone_vdp(counts)
    assert v.shape == (2, 3) and v.dtype == np.float64
    assert v[0, 1] == 25.0 and v[1, 2] == 100.0 and np.isnan(v[0, 0]) and np.isnan(v[1, 1])
    stats = np.array([[4, 0, 0, 3 << 24], [0, 1, 2, 0]], np.int64)
    m = _lib.zone_mean(stats)
    assert m[0] == 0.75 and np.isnan(m[1])


def test_regional_vdp_needs_calculate_vdp():
    """Called before calculate_VDP it raises; no device is touched and the object stays as it was."""
    from vent_analysis_amd import Vent_Analysis
    X, M = DR.D.field((7, 5, 3), 1)
    va = Vent_Analysis(pickle_dict=dict(HPvent=X, mask=M.astype(np.float64), vox=[1.5, 1.5, 10.0]))
    assert hasattr(Vent_Analysis, "regional_vdp") and "sets nothing on the object" in Vent_Analysis.regional_vdp.__doc__
    before = {k: (v.copy() if isinstance(v, (np.ndarray, dict)) else v) for k, v in vars(va).items()}
    with pytest.raises(ValueError):
        va.regional_vdp()
    with pytest.raises(ValueError):
        va.regional_vdp(parts=(2, 2, 1), lateral=False)
    assert set(vars(va)) == set(before)
    np.testing.assert_equal({k: v for k, v in vars(va).items()}, before)
    assert isinstance(va.N4HPvent, str) and isinstance(va.defectArray, str)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_state_and_rule_under_sanitizers(tmp_path):
    exe = str(tmp_path / "chk")
    subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(REPO, "tests", "zones_state_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "zones state ok" in r.stdout, r.stdout + r.stderr


def test_design_has_the_state_row():
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert "`zones_enqueued(k, bins)`" in design and "`need_zones()`" in design


# ---- the reference itself ------------------------------------------------------------------------
PROTOTYPE_SHAPES = [(7, 5, 3), (12, 9, 1), (41, 37, 9), (33, 20, 5), (64, 64, 24), (130, 19, 2)]


@pytest.mark.parametrize("bridge", [False, True], ids=["gap", "bridge"])
@pytest.mark.parametrize("shape", PROTOTYPE_SHAPES, ids=str)
def test_the_partition_finds_the_gap_and_leaves_no_zone_empty(shape, bridge):
    m = R.lungs(shape, bridge)
    g0, g1 = R.gap(shape)
    Pc = R.profiles(m)[1]
    assert not Pc[g0:g1].any() if not bridge else (Pc[g0:g1] == shape[2]).all()
    assert R.split(Pc) == g0                                          # the gap's first column: ties go left
    parts = (3, 1, min(2, shape[2]))
    for by in BYS:
        zm = R.zone_map(m, parts, True, by)
        K = R.n_zones(parts, True)
        n = np.bincount(zm[m != 0], minlength=K + 1)
        assert n[0] == 0 and (n[1:] > 0).all(), (by, n)
        assert not zm[m == 0].any()
        side = (zm.astype(int) - 1) // parts[2] % 2
        assert (side[:, :g0][m[:, :g0] != 0] == 0).all() and (side[:, g0:][m[:, g0:] != 0] == 1).all()


@pytest.mark.parametrize("norm,bins,hi", [("mean", 100, 1.5), ("p99", 7, 2.0)])
@pytest.mark.parametrize("shape", [(41, 37, 9), (7, 5, 3)], ids=str)
def test_reference_identities(shape, norm, bins, hi):
    """Summed over zones the histogram is the distribution's and counts[:, 0] the mask count; the
    negated values fill n_below, the all-zero signal n_over."""
    hp, mk = R.batch_inputs(shape)
    defect, lb = R.batch_maps(shape)
    rng = np.random.default_rng(3)
    for q in range(hp.shape[0]):
        labels = rng.integers(0, 9, shape).astype(np.uint8)
        for kw in (dict(parts=(3, 1, 1), lateral=True, by=R.EXTENT), dict(parts=(2, 3, 2), lateral=False, by=R.COUNT),
                   dict(labels=labels, K=5)):
            r = R.reference(hp[q], mk[q], defect[q], lb[q], norm=norm, bins=bins, hi=hi, **kw)
            h, outside = DR.histogram(hp[q], mk[q], norm, bins, hi)
            n_mask = int((mk[q] != 0).sum())
            assert np.array_equal(r["hist"].sum(axis=0, dtype=np.uint32), h), q
            assert np.array_equal(r["stats"][:, 1:3].sum(axis=0), outside), q
            assert np.array_equal(r["stats"][:, 0], r["hist"].sum(axis=1)), q
            assert int(r["counts"][:, 0].sum()) == n_mask == int(r["stats"][:, :3].sum()), q
            assert np.array_equal(r["counts"].sum(axis=0), DR.slice_counts(mk[q], defect[q] * (mk[q] != 0), lb[q]).sum(axis=0))
            assert np.array_equal(r["counts"][:, 0], np.bincount(r["map"][mk[q] != 0], minlength=r["counts"].shape[0]))
            if "labels" in kw:
                assert r["geom"][6] == -1 and (r["counts"][0, 0] > 0) == bool(n_mask)   # labels 0 and 6..8: unassigned
            else:
                assert r["counts"][0].sum() == 0 and r["hist"][0].sum() == 0
    refs = [R.reference(hp[q], mk[q], defect[q], lb[q], norm=norm, bins=bins, hi=hi) for q in (2, 4, 5, 6)]
    assert not refs[0]["counts"].any() and list(refs[0]["geom"]) == [0, -1, 0, -1, 0, -1, 0, 0]   # the empty mask
    assert refs[1]["counts"][[1, 3, 5], 0].sum() == 0 and refs[1]["geom"][6] == shape[1] // 2    # side 0 is empty
    assert refs[2]["stats"][:, 1].sum() > 0                                                         # negated values
    assert refs[3]["stats"][:, 2].sum() == int((mk[6] != 0).sum()) and not refs[3]["hist"].any()    # NaN
