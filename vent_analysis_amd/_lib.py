"""ctypes binding of libventhip.so (include/vent_hip.h).

The library is built in-tree (``python __graft_entry__.py`` / ``make -C vent_analysis_amd/csrc``)
and MUST be present: there is no CPU fallback.  Every status code is mapped to the Python
exception the reference raises at the same point (SURVEY.md §8b "Errors").
"""
from __future__ import annotations

import atexit
import ctypes as ct
import os
import threading
import weakref

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VH_LIB_PATH") or os.path.join(HERE, "libventhip.so")   # override: A/B builds

VH_OK, VH_ERR_ARG, VH_ERR_HIP, VH_ERR_NOMEM, VH_ERR_MAXRADIUS, VH_ERR_EMPTY, VH_ERR_RCCL, \
    VH_ERR_NODEV, VH_ERR_INDEX = range(9)
COHORT_BINS = 1024
COMM_ID_BYTES = 128
VH_DEFECT_MEAN, VH_DEFECT_LB, VH_DEFECT_KM = range(3)   # vh_batch_select_defect sources
_DEFECT_SOURCES = {"mean": VH_DEFECT_MEAN, "lb": VH_DEFECT_LB, "kmeans": VH_DEFECT_KM}


def defect_source(source) -> int:
    """'mean' | 'lb' | 'kmeans' or the VH_DEFECT_* ints -> the int; anything else raises ValueError."""
    if isinstance(source, str):
        if source not in _DEFECT_SOURCES:
            raise ValueError(f"defect source is 'mean', 'lb' or 'kmeans', got {source!r}")
        return _DEFECT_SOURCES[source]
    if isinstance(source, (bool, float)) or int(source) != source:
        raise ValueError(f"defect source is 'mean', 'lb' or 'kmeans' or 0..2, got {source!r}")
    return int(source)   # (the library checks the range)


VH_NORM_MEAN, VH_NORM_P99 = range(2)   # vh_batch_distribution: the divisor of the normalised signal
VH_DIST_COLS = 8                       # slice_counts columns: mask, defect, LB class 1..6
_NORM_SOURCES = {"mean": VH_NORM_MEAN, "p99": VH_NORM_P99}


def norm_source(norm) -> int:
    """'mean' | 'p99' or the VH_NORM_* ints -> the int; anything else raises ValueError."""
    if isinstance(norm, str):
        if norm not in _NORM_SOURCES:
            raise ValueError(f"norm is 'mean' or 'p99', got {norm!r}")
        return _NORM_SOURCES[norm]
    if isinstance(norm, (bool, float)) or int(norm) != norm:
        raise ValueError(f"norm is 'mean' or 'p99' or 0..1, got {norm!r}")
    return int(norm)   # (the library checks the range)


def dist_edges(bins, hi):
    """The histogram's bin edges for display: float64 [bins + 1], arange(bins + 1) * (hi / bins)."""
    return np.arange(int(bins) + 1) * (float(hi) / int(bins))


VH_MASK_ERODE, VH_MASK_DILATE, VH_MASK_OPEN, VH_MASK_CLOSE = range(4)   # vh_batch_edit_mask ops
VH_PAINT_OR, VH_PAINT_ANDNOT, VH_PAINT_AND, VH_PAINT_XOR = range(4)     # vh_batch_paint_mask modes
_MASK_OPS = {"erode": VH_MASK_ERODE, "dilate": VH_MASK_DILATE, "open": VH_MASK_OPEN, "close": VH_MASK_CLOSE}
_PAINT_MODES = {"or": VH_PAINT_OR, "andnot": VH_PAINT_ANDNOT, "and": VH_PAINT_AND, "xor": VH_PAINT_XOR}


def _named_int(value, names, what):
    """A name of ``names`` or one of its ints -> the int; anything else raises ValueError."""
    if isinstance(value, str):
        if value not in names:
            raise ValueError(f"{what} is one of {sorted(names)}, got {value!r}")
        return names[value]
    if isinstance(value, (bool, float)) or not isinstance(value, (int, np.integer)) \
            or int(value) not in names.values():
        raise ValueError(f"{what} is one of {sorted(names)} or 0..{len(names) - 1}, got {value!r}")
    return int(value)


def paint_mode(how) -> int:
    """'or' | 'andnot' | 'and' | 'xor' or the VH_PAINT_* ints -> the int; else ValueError."""
    return _named_int(how, _PAINT_MODES, "paint mode")


def _mask_edit_args(op, radius, n):
    """(op int, radius int32 [n] contiguous) for vh_batch_edit_mask: ``op`` 'erode' | 'dilate' | 'open'
    | 'close' or the VH_MASK_* ints, ``radius`` a scalar or one int per study, each 0..5.  ValueError
    for what the library would refuse, so the message names the argument."""
    op = _named_int(op, _MASK_OPS, "mask op")
    r = np.asarray(radius)
    if r.dtype == np.bool_ or not np.issubdtype(r.dtype, np.integer):
        raise ValueError(f"edit_mask: radius is an int or one int per study, got {radius!r}")
    if r.ndim > 1 or (r.ndim == 1 and r.shape[0] != n):
        raise ValueError(f"edit_mask: {n} studies, got radius of shape {r.shape}")
    if r.size and (r.min() < 0 or r.max() > 5):
        raise ValueError(f"edit_mask: every radius must be 0..5, got {radius!r}")
    return op, np.ascontiguousarray(np.broadcast_to(r, (n,)), dtype=np.int32)


SEG_MAX_PLANE = 512   # vh_batch_segment takes planes of at most 512 x 512


def _segment_args(thresh, open_radius, n, shape=None):
    """(thresh float32 [n] contiguous or None, open_radius int32 [n] contiguous) for vh_batch_segment:
    ``thresh`` None (Otsu), a scalar or one value per study, each finite and > 0; ``open_radius`` a
    scalar or one int per study, each 0..5; ``shape`` (R, C, Z), a plane of at most 512 x 512.
    ValueError for what the library would refuse, so the message names the argument."""
    if shape is not None and (shape[0] > SEG_MAX_PLANE or shape[1] > SEG_MAX_PLANE):
        raise ValueError(f"segment: a plane of at most {SEG_MAX_PLANE} x {SEG_MAX_PLANE}, got {tuple(shape)[:2]}")
    r = np.asarray(open_radius)
    if r.dtype == np.bool_ or not np.issubdtype(r.dtype, np.integer):
        raise ValueError(f"segment: open_radius is an int or one int per study, got {open_radius!r}")
    if r.ndim > 1 or (r.ndim == 1 and r.shape[0] != n):
        raise ValueError(f"segment: {n} studies, got open_radius of shape {r.shape}")
    if r.size and (r.min() < 0 or r.max() > 5):
        raise ValueError(f"segment: every open_radius must be 0..5, got {open_radius!r}")
    rad = np.ascontiguousarray(np.broadcast_to(r, (n,)), dtype=np.int32)
    if thresh is None:
        return None, rad
    t = np.asarray(thresh)
    if t.dtype == np.bool_ or not (np.issubdtype(t.dtype, np.floating) or np.issubdtype(t.dtype, np.integer)):
        raise ValueError(f"segment: thresh is a number or one per study, got {thresh!r}")
    if t.ndim > 1 or (t.ndim == 1 and t.shape[0] != n):
        raise ValueError(f"segment: {n} studies, got thresh of shape {t.shape}")
    th = np.ascontiguousarray(np.broadcast_to(t.astype(np.float32), (n,)))
    bad = np.flatnonzero(~(np.isfinite(th) & (th > 0)))
    if bad.size:
        raise ValueError(f"segment: every thresh must be finite and > 0 (studies {bad.tolist()}: "
                         f"{th[bad].tolist()})")
    return th, rad


def otsu(hist):
    """The Otsu cut of a histogram (vh_otsu, on the host: no device): the lowest k in 0 .. len - 2 that
    maximises the between-class variance of bins <= k against bins > k.  IndexError when fewer than
    two bins are occupied."""
    h = np.ascontiguousarray(hist, dtype=np.uint32)
    if h.ndim != 1 or h.size < 2:
        raise ValueError("otsu: a 1-D histogram of at least two bins")
    k = ct.c_int32(-1)
    rc = lib().vh_otsu(_ptr(h), h.size, ct.byref(k))
    if rc == VH_ERR_EMPTY:
        raise IndexError("vh_otsu: fewer than two occupied bins")
    if rc != VH_OK:
        raise ValueError(f"vh_otsu: status {rc}")
    return int(k.value)


VH_SHIFT_PROTON, VH_SHIFT_MASK = range(2)   # vh_batch_shift targets
REG_MAX_SEARCH = (8, 8, 2)                  # vh_batch_register: the largest search window
REG_LEVELS = 32                             # its joint histograms are [32][32]


def _register_args(search, shape):
    """search -> int32 [3] contiguous for vh_batch_register: three ints (Sr, Sc, Sz) with 0 <= Sr, Sc <= 8,
    0 <= Sz <= 2 and each below its dimension of ``shape`` (R, C, Z).  ValueError for what the library
    would refuse, so the message names the argument."""
    s = np.asarray(search)
    if s.dtype == np.bool_ or not np.issubdtype(s.dtype, np.integer) or s.shape != (3,):
        raise ValueError(f"register: search is three ints (Sr, Sc, Sz), got {search!r}")
    for k, (v, hi, n) in enumerate(zip(s.tolist(), REG_MAX_SEARCH, tuple(shape)[-3:])):
        if v < 0 or v > hi or v >= n:
            raise ValueError(f"register: search[{k}] must be 0..{hi} and below the dimension {n}, got {search!r}")
    return np.ascontiguousarray(s, dtype=np.int32)


def _shift_args(shifts, n, shape):
    """shifts -> int32 [n][3] contiguous for vh_batch_shift: one (dr, dc, dz) for every study or one per
    study, each |component| at most its dimension of ``shape`` (R, C, Z)."""
    s = np.asarray(shifts)
    if s.dtype == np.bool_ or not np.issubdtype(s.dtype, np.integer) or s.shape not in ((3,), (n, 3)):
        raise ValueError(f"shift: {n} studies take (dr, dc, dz) or one per study, got {shifts!r}")
    s = np.ascontiguousarray(np.broadcast_to(s, (n, 3)), dtype=np.int32)
    if s.size and (np.abs(s.astype(np.int64)) > np.asarray(tuple(shape)[-3:], np.int64)).any():
        raise ValueError(f"shift: every |shift| is at most its dimension of {tuple(shape)[-3:]}, got {shifts!r}")
    return s


def mi(joint):
    """The mutual information of a square joint histogram (vh_mi, on the host: no device), float64: the
    sums as exact integers, every term J log((J n) / (Ja Jb)) in double, 0.0 for an empty histogram."""
    j = np.ascontiguousarray(joint, dtype=np.uint32)
    if j.ndim != 2 or j.shape[0] != j.shape[1] or not 1 <= j.shape[0] <= 256:
        raise ValueError("mi: a square histogram of 1..256 levels")
    out = ct.c_double(0.0)
    rc = lib().vh_mi(_ptr(j), j.shape[0], ct.byref(out))
    if rc != VH_OK:
        raise ValueError(f"vh_mi: status {rc}")
    return float(out.value)


def register_pick(score, search):
    """The best shift (dr, dc, dz) of one study's scores (vh_register_pick, on the host): the largest
    score, among equal scores the smallest |dr| + |dc| + |dz|, then the lowest index.  ``score`` is
    [2Sz+1][2Sr+1][2Sc+1] or flat in that order."""
    s = np.asarray(search)
    if s.shape != (3,) or not np.issubdtype(s.dtype, np.integer):
        raise ValueError(f"register_pick: search is three ints, got {search!r}")
    se = _register_args(search, (1 << 30,) * 3)
    sc = np.ascontiguousarray(score, dtype=np.float64)
    ns = int(np.prod(2 * se + 1))
    if sc.size != ns:
        raise ValueError(f"register_pick: search {tuple(se.tolist())} has {ns} shifts, got {sc.size} scores")
    best = np.zeros(3, np.int32)
    rc = lib().vh_register_pick(_ptr(sc), _ptr(se), _ptr(best))
    if rc != VH_OK:
        raise ValueError(f"vh_register_pick: status {rc}")
    return tuple(int(v) for v in best)


def _score_shape(search):
    return (2 * int(search[2]) + 1, 2 * int(search[0]) + 1, 2 * int(search[1]) + 1)


RESAMPLE_TAPS = 8                           # VH_RESAMPLE_TAPS: taps of one axis at most
RESAMPLE_MAX_SRC = 1024                     # the largest source dimension
RESAMPLE_SCALE = (0.25, 4.0)                # the limits of a map's scale
RESAMPLE_MAX_OFFSET = float(1 << 20)        # ... and of |offset|


def _real_array(a, what):
    x = np.asarray(a)
    if x.dtype == np.bool_ or not (np.issubdtype(x.dtype, np.floating) or np.issubdtype(x.dtype, np.integer)):
        raise ValueError(f"{what}: numbers, got {a!r}")
    return x.astype(np.float64)


def _shape3(shape, what, hi=None):
    s = np.asarray(shape)
    if s.dtype == np.bool_ or not np.issubdtype(s.dtype, np.integer) or s.shape != (3,):
        raise ValueError(f"{what} is three ints, got {shape!r}")
    if (s < 1).any() or (hi is not None and (s > hi).any()):
        raise ValueError(f"{what}: every dimension must be 1..{hi if hi is not None else ''}, got {shape!r}")
    return tuple(int(v) for v in s)


def resample_taps(n_src, n_dst, scale, offset):
    """The tap table of one axis of the resampler (vh_resample_taps, on the host: no device; the spec is in
    include/vent_hip.h): destination index i looks at source coordinate scale * i + offset.  Returns
    (first int32 [n_dst], count int32 [n_dst], weight float32 [n_dst][8])."""
    n_src, n_dst = int(n_src), int(n_dst)
    if n_dst < 1:
        raise ValueError(f"resample_taps: n_dst must be >= 1, got {n_dst}")
    first, count = np.zeros(n_dst, np.int32), np.zeros(n_dst, np.int32)
    weight = np.zeros((n_dst, RESAMPLE_TAPS), np.float32)
    rc = lib().vh_resample_taps(n_src, n_dst, float(scale), float(offset), _ptr(first), _ptr(count), _ptr(weight))
    if rc != VH_OK:
        raise ValueError(f"resample_taps: n_src 1..{RESAMPLE_MAX_SRC}, scale in {list(RESAMPLE_SCALE)}, |offset| <= 2^20, "
                         f"got n_src {n_src}, n_dst {n_dst}, scale {scale!r}, offset {offset!r}")
    return first, count, weight


def grid_map(src_shape, src_vox, dst_shape, dst_vox, shift=(0, 0, 0)):
    """The map float64 [3][2] of (scale, offset) per axis that puts the fields of view of two grids centre
    on centre: scale = dst_vox / src_vox and offset = (n_src - 1) / 2 - scale * (n_dst - 1) / 2 + scale * shift.
    ``shift`` is in destination voxels, so a registration's best shift can be folded into the map: the
    result is the unshifted resampling moved as vh_batch_shift moves it, with the source's own data in the
    margin instead of zeros."""
    ns = np.asarray(_shape3(src_shape, "grid_map: src_shape"), np.float64)
    nd = np.asarray(_shape3(dst_shape, "grid_map: dst_shape"), np.float64)
    vs, vd, sh = (_real_array(v, "grid_map: " + k) for v, k in ((src_vox, "src_vox"), (dst_vox, "dst_vox"),
                                                                (shift, "shift")))
    if vs.shape != (3,) or vd.shape != (3,) or sh.shape != (3,):
        raise ValueError("grid_map: src_vox, dst_vox and shift have three values each")
    if not (np.isfinite(vs).all() and np.isfinite(vd).all() and (vs > 0).all() and (vd > 0).all()):
        raise ValueError(f"grid_map: voxel sizes must be finite and > 0, got {src_vox!r} and {dst_vox!r}")
    scale = vd / vs
    offset = (ns - 1.0) / 2.0 - scale * (nd - 1.0) / 2.0 + scale * sh
    return np.ascontiguousarray(np.stack([scale, offset], axis=1))


def _resample_args(maps, n, src_shape=None):
    """maps -> float64 [n][3][2] contiguous for vh_batch_resample_proton: one [3][2] map of (scale, offset)
    per axis for every study, or one per study; every scale finite in [0.25, 4] and every offset finite
    with |offset| <= 2^20.  ``src_shape`` (Rs, Cs, Zs), each 1..1024, is checked when given.  ValueError
    for what the library would refuse, so the message names the argument."""
    if src_shape is not None:
        _shape3(src_shape, "resample: the source shape", RESAMPLE_MAX_SRC)
    m = _real_array(maps, "resample: maps")
    if m.shape not in ((3, 2), (n, 3, 2)):
        raise ValueError(f"resample: {n} studies take a [3][2] map or one per study, got shape {m.shape}")
    m = np.ascontiguousarray(np.broadcast_to(m, (n, 3, 2)))
    s, o = m[..., 0], m[..., 1]
    with np.errstate(invalid="ignore"):
        ok = (s >= RESAMPLE_SCALE[0]) & (s <= RESAMPLE_SCALE[1]) & (np.abs(o) <= RESAMPLE_MAX_OFFSET)
    if not ok.all():
        raise ValueError(f"resample: every scale in {list(RESAMPLE_SCALE)} and every |offset| <= 2^20, both finite "
                         f"(studies {sorted(set(np.argwhere(~ok)[:, 0].tolist()))})")
    return m


RM_MAX_COUNT = (17, 17, 5)                  # vh_batch_register_maps: the most candidates of the r, c and z lists
RM_FACTORS = (0.94, 0.97, 1.0, 1.03, 1.06)  # map_candidates: the scale factors of the in-plane axes
RM_SHIFTS = (-0.5, 0.0, 0.5)                # ... and the shifts of every axis, in destination voxels


def axis_candidates(base, n_dst, factors, shifts):
    """The candidate list of one axis for register_maps (vh_axis_candidates, on the host: no device; the
    spec is in include/vent_hip.h): around ``base`` (scale0, offset0), factor f scales about the centre of
    the ``n_dst`` destination voxels and shift d, in destination voxels, moves.  Entry fi * len(shifts) + si is
    scale = scale0 * f, offset = offset0 + scale0 * ((n_dst - 1) / 2 * (1 - f) + d).  Returns float64
    [len(factors) * len(shifts)][2]; ValueError for an empty list or a result outside the resampler's limits."""
    b = _real_array(base, "axis_candidates: base")
    f = np.ascontiguousarray(_real_array(factors, "axis_candidates: factors"))
    d = np.ascontiguousarray(_real_array(shifts, "axis_candidates: shifts"))
    if b.shape != (2,) or f.ndim != 1 or d.ndim != 1 or not f.size or not d.size:
        raise ValueError("axis_candidates: base is (scale, offset), factors and shifts are non-empty 1-D lists")
    out = np.zeros((f.size * d.size, 2), np.float64)
    rc = lib().vh_axis_candidates(float(b[0]), float(b[1]), int(n_dst), _ptr(f), f.size, _ptr(d), d.size, _ptr(out))
    if rc != VH_OK:
        raise ValueError(f"axis_candidates: n_dst 1..2^20 and every candidate's scale in {list(RESAMPLE_SCALE)}, "
                         f"|offset| <= 2^20, got base {base!r}, n_dst {n_dst!r}, factors {factors!r}, shifts {shifts!r}")
    return out


def _home_of(values, one):
    v = np.asarray(values, np.float64)
    at = np.flatnonzero(v == one)
    return int(at[0]) if at.size else None


def map_candidates(base_map, dst_shape, factors=RM_FACTORS, shifts=RM_SHIFTS, zfactors=(1.0,), zshifts=RM_SHIFTS):
    """The three candidate lists of register_maps around one map [3][2] (grid_map makes one): the r and the
    c axis take ``factors`` x ``shifts``, the z axis ``zfactors`` x ``zshifts`` (axis_candidates).  Returns
    (lists, home): lists the r, c and z list, float64 [K][2] each; home the entry of each list that is the
    base itself (factor 1.0 and shift 0.0), or the middle entry where a list has none."""
    m = _real_array(base_map, "map_candidates: base_map")
    if m.shape != (3, 2):
        raise ValueError(f"map_candidates: base_map is [3][2], got shape {m.shape}")
    n = _shape3(dst_shape, "map_candidates: dst_shape")
    lists, home = [], []
    for a in range(3):
        fa, sa = (zfactors, zshifts) if a == 2 else (factors, shifts)
        lists.append(axis_candidates(m[a], n[a], fa, sa))
        fi, si = _home_of(fa, 1.0), _home_of(sa, 0.0)
        home.append(fi * len(sa) + si if fi is not None and si is not None else (len(lists[-1]) - 1) // 2)
    return lists, tuple(home)


def _register_maps_args(lists, n, home=None):
    """(count int32 [3], axis_maps float64 [n][Kr+Kc+Kz][2] contiguous, home int32 [3] or None) for
    vh_batch_register_maps: ``lists`` is the r, the c and the z list, each [K][2] of (scale, offset) for
    every study or [n][K][2], one per study; 1 <= Kr, Kc <= 17, 1 <= Kz <= 5; every scale finite in
    [0.25, 4] and every offset finite with |offset| <= 2^20; ``home`` three ints inside the lists.
    ValueError for what the library would refuse, so the message names the argument."""
    if isinstance(lists, np.ndarray) or len(lists) != 3:
        raise ValueError("register_maps: lists is the r, the c and the z list")
    parts = []
    for a, (l, hi) in enumerate(zip(lists, RM_MAX_COUNT)):
        m = _real_array(l, f"register_maps: lists[{a}]")
        if m.ndim == 2:
            m = np.broadcast_to(m, (n,) + m.shape)
        if m.ndim != 3 or m.shape[0] != n or m.shape[2] != 2:
            raise ValueError(f"register_maps: lists[{a}] is [K][2] or [{n}][K][2], got shape {np.shape(l)}")
        if not 1 <= m.shape[1] <= hi:
            raise ValueError(f"register_maps: lists[{a}] has 1..{hi} candidates, got {m.shape[1]}")
        parts.append(m)
    am = np.ascontiguousarray(np.concatenate(parts, axis=1))
    s, o = am[..., 0], am[..., 1]
    with np.errstate(invalid="ignore"):
        ok = (s >= RESAMPLE_SCALE[0]) & (s <= RESAMPLE_SCALE[1]) & (np.abs(o) <= RESAMPLE_MAX_OFFSET)
    if not ok.all():
        raise ValueError(f"register_maps: every scale in {list(RESAMPLE_SCALE)} and every |offset| <= 2^20, both finite "
                         f"(studies {sorted(set(np.argwhere(~ok)[:, 0].tolist()))})")
    count = np.asarray([q.shape[1] for q in parts], np.int32)
    return count, am, _home_args(home, count)


def _home_args(home, count):
    if home is None:
        return None
    h = np.asarray(home)
    if h.dtype == np.bool_ or not np.issubdtype(h.dtype, np.integer) or h.shape != (3,):
        raise ValueError(f"register_maps: home is three ints, got {home!r}")
    if (h < 0).any() or (h >= np.asarray(count)).any():
        raise ValueError(f"register_maps: home must lie inside the lists of {tuple(int(v) for v in count)} "
                         f"candidates, got {home!r}")
    return np.ascontiguousarray(h, dtype=np.int32)


def register_maps_pick(score, home=None, count=None):
    """The best candidate (kr, kc, kz) of one study's scores (vh_register_maps_pick, on the host): the
    largest score, among equal scores the smallest |kr - hr| + |kc - hc| + |kz - hz|, then the lowest
    index; a NaN never wins.  ``score`` is [Kz][Kr][Kc], or flat in that order with ``count`` (Kr, Kc, Kz);
    ``home`` defaults to the middle entry of each list."""
    sc = np.ascontiguousarray(score, dtype=np.float64)
    if count is None:
        if sc.ndim != 3:
            raise ValueError("register_maps_pick: score is [Kz][Kr][Kc], or flat with count")
        count = (sc.shape[1], sc.shape[2], sc.shape[0])
    c = np.asarray(count)
    if c.dtype == np.bool_ or not np.issubdtype(c.dtype, np.integer) or c.shape != (3,):
        raise ValueError(f"register_maps_pick: count is three ints, got {count!r}")
    if (c < 1).any() or (c > np.asarray(RM_MAX_COUNT)).any():
        raise ValueError(f"register_maps_pick: count must be 1..17, 1..17, 1..5, got {count!r}")
    cn = np.ascontiguousarray(c, dtype=np.int32)
    if sc.size != int(np.prod(cn)):
        raise ValueError(f"register_maps_pick: count {tuple(cn.tolist())} has {int(np.prod(cn))} candidates, got "
                         f"{sc.size} scores")
    h = _home_args(home, cn)
    best = np.zeros(3, np.int32)
    rc = lib().vh_register_maps_pick(_ptr(sc), _ptr(cn), _ptr(h), _ptr(best))
    if rc != VH_OK:
        raise ValueError(f"vh_register_maps_pick: status {rc}")
    return tuple(int(v) for v in best)


def denoise_constants(sigma, strength=2.0, patch=1):
    """(inv_h2, bias) float32 of one study as vh_batch_denoise forms them: in double from the float32
    sigma and strength, rounded once.  inv_h2 = 1 / (2 n (k sigma)^2), n = (2 patch + 1)^2; bias =
    2 sigma^2."""
    s, k = np.float64(np.float32(sigma)), np.float64(np.float32(strength))
    ks = k * s
    with np.errstate(divide="ignore", over="ignore"):
        return (np.float32(np.float64(1.0) / (2.0 * np.float64((2 * int(patch) + 1) ** 2) * (ks * ks))),
                np.float32(2.0 * (s * s)))


class N4Params(ct.Structure):
    _fields_ = [("n_levels", ct.c_int32), ("max_iters", ct.c_int32 * 8),
                ("conv_threshold", ct.c_float), ("ncp", ct.c_int32 * 3),
                ("spline_order", ct.c_int32), ("n_bins", ct.c_int32),
                ("wiener_noise", ct.c_float), ("fwhm", ct.c_float), ("conv_mode", ct.c_int32)]


class VdpResult(ct.Structure):
    _fields_ = [("vdp", ct.c_double), ("vdp_lb", ct.c_double), ("vdp_km", ct.c_double),
                ("defect_volume", ct.c_double), ("lung_volume", ct.c_double),
                ("km_centres", ct.c_double * 4), ("snr", ct.c_double),
                ("mean_anchor", ct.c_float), ("p99", ct.c_float),
                ("n_mask", ct.c_int64), ("n_defect", ct.c_int64), ("n_lb12", ct.c_int64),
                ("n_km0", ct.c_int64), ("n4_iters", ct.c_int32 * 8), ("n4_conv", ct.c_float * 8)]


class RunOpts(ct.Structure):
    _fields_ = [("do_n4", ct.c_int32), ("n4", N4Params), ("thresh", ct.c_float),
                ("do_snr", ct.c_int32), ("do_kmeans", ct.c_int32), ("do_cohort", ct.c_int32),
                ("profile", ct.c_int32), ("vox", ct.c_double * 3), ("n4_subbatch", ct.c_int32),
                ("morph3d", ct.c_int32), ("n4_mode", ct.c_int32)]


class VentHipError(RuntimeError):
    pass


_P = ct.c_void_p
_I64 = ct.c_int64
_SIGS = {
    "vh_abi_version": ([], ct.c_int),
    "vh_status_string": ([ct.c_int], ct.c_char_p),
    "vh_device_count": ([ct.POINTER(ct.c_int)], ct.c_int),
    "vh_n4_default_params": ([ct.POINTER(N4Params)], None),
    "vh_default_run_opts": ([ct.POINTER(RunOpts)], None),
    "vh_create": ([ct.c_int, ct.POINTER(_P)], ct.c_int),
    "vh_destroy": ([_P], ct.c_int),
    "vh_last_error": ([_P], ct.c_char_p),
    "vh_synchronize": ([_P], ct.c_int),
    "vh_n4": ([_P, _P, _P, _I64, _I64, _I64, _I64, ct.POINTER(N4Params), _P, _P, _P], ct.c_int),
    "vh_border": ([_P, _P, _I64, _I64, _I64, _I64, _P], ct.c_int),
    "vh_snr": ([_P, _P, _P, _I64, _I64, _I64, _I64, _P], ct.c_int),
    "vh_vdp": ([_P, _P, _P, _P, _I64, _I64, _I64, _I64, ct.c_float, _P, _P, _P, _P, _P], ct.c_int),
    "vh_ci": ([_P, _P, _I64, _I64, _I64, _I64, _P, _P, _I64, _P, _P, _I64, ct.c_double, _P, _P,
               _P], ct.c_int),
    "vh_ci_table_create": ([_P, _I64, _I64, _P, _P, _I64, _P, _P, _I64, ct.POINTER(_P)], ct.c_int),
    "vh_ci_table_destroy": ([_P], ct.c_int),
    "vh_ci_tab": ([_P, _P, _I64, _I64, _I64, _I64, _P, ct.c_double, _P, _P, _P], ct.c_int),
    "vh_batch_create": ([_P, _I64, _I64, _I64, _I64, ct.POINTER(_P)], ct.c_int),
    "vh_batch_destroy": ([_P], ct.c_int),
    "vh_batch_upload": ([_P, _P, _P], ct.c_int),
    "vh_batch_run": ([_P, ct.POINTER(RunOpts)], ct.c_int),
    "vh_batch_sync": ([_P], ct.c_int),
    "vh_batch_download": ([_P, _P, _P, _P, _P, _P], ct.c_int),
    "vh_batch_ci": ([_P, _P, ct.c_double], ct.c_int),
    "vh_batch_set_defect": ([_P, _P], ct.c_int),
    "vh_batch_download_ci": ([_P, _P, _P, _P, _P], ct.c_int),
    "vh_batch_select_defect": ([_P, ct.c_int, ct.c_int], ct.c_int),
    "vh_batch_download_defect": ([_P, _P, _P, _P, _P], ct.c_int),
    "vh_batch_km_cuts": ([_P, _P], ct.c_int),
    "vh_defect_map": ([_P, _P, _P, _I64, _I64, _I64, _I64, ct.c_float, ct.c_int, ct.c_int, _P, _P, _P,
                       _P], ct.c_int),
    "vh_batch_cohort_hist": ([_P, _P], ct.c_int),
    "vh_batch_kernel_names": ([], ct.c_char_p),
    "vh_batch_reset_timers": ([_P], ct.c_int),
    "vh_batch_kernel_time": ([_P, ct.c_char_p, ct.POINTER(ct.c_double), ct.POINTER(ct.c_int64),
                              ct.POINTER(ct.c_double)], ct.c_int),
    "vh_batch_study_times": ([_P, _P], ct.c_int),
    "vh_ctx_profile": ([_P, ct.c_int], ct.c_int),
    "vh_ctx_kernel_time": ([_P, ct.c_char_p, ct.POINTER(ct.c_double), ct.POINTER(ct.c_int64)],
                           ct.c_int),
    "vh_overlay": ([_P, _P, _P, _I64, _I64, _I64, _I64, _P], ct.c_int),
    "vh_montage": ([_P, _I64, _I64, _I64, _P, ct.c_int, _P, ct.c_int, _P, _P, _P, _P, _P, _I64, _P,
                    _P], ct.c_int),
    "vh_batch_overlay": ([_P], ct.c_int),
    "vh_batch_download_overlay": ([_P, _P], ct.c_int),
    "vh_batch_montage_layout": ([_P, _P, _P, _P], ct.c_int),
    "vh_batch_montage": ([_P, _P, _P, _I64], ct.c_int),
    "vh_batch_download_montage": ([_P, _P, _P], ct.c_int),
    "vh_batch_distribution": ([_P, ct.c_int, ct.c_int32, ct.c_float], ct.c_int),
    "vh_batch_download_distribution": ([_P, _P, _P, _P], ct.c_int),
    "vh_distribution": ([_P, _P, _P, _I64, _I64, _I64, _I64, ct.c_float, ct.c_int, ct.c_int32, ct.c_float,
                         _P, _P, _P], ct.c_int),
    "vh_batch_heterogeneity": ([_P, ct.c_int, ct.c_int32, ct.c_int32, ct.c_float, ct.c_int], ct.c_int),
    "vh_batch_download_heterogeneity": ([_P, _P, _P, _P], ct.c_int),
    "vh_heterogeneity": ([_P, _P, _P, _I64, _I64, _I64, _I64, ct.c_int, ct.c_int32, ct.c_int32, ct.c_float,
                          _P, _P, _P], ct.c_int),
    "vh_batch_core_rind": ([_P, _P, ct.c_int32, ct.c_int], ct.c_int),
    "vh_batch_download_core_rind": ([_P, _P, _P, _P], ct.c_int),
    "vh_core_rind_form": ([_I64, _I64, _I64], ct.c_int),
    "vh_core_rind": ([_P, _P, _P, _I64, _I64, _I64, _I64, _P, ct.c_int32, _P, _P, _P], ct.c_int),
    "vh_batch_components": ([_P, ct.c_int, ct.c_int, _P, ct.c_int32], ct.c_int),
    "vh_batch_download_components": ([_P, _P, _P, _P, _P], ct.c_int),
    "vh_batch_filter_components": ([_P, ct.c_int, ct.c_int, _P, _P, _P], ct.c_int),
    "vh_batch_defect_table": ([_P, _P, ct.c_int32, ct.c_int], ct.c_int),
    "vh_batch_download_defect_table": ([_P, _P, _P], ct.c_int),
    "vh_components": ([_P, _P, _I64, _I64, _I64, _I64, ct.c_int, _P, ct.c_int32, _P, _P, _P, _P], ct.c_int),
    "vh_filter_components": ([_P, _P, _I64, _I64, _I64, _I64, ct.c_int, _P, _P, _P, _P], ct.c_int),
    "vh_zone_parts": ([_P, _I64, ct.c_int32, ct.c_int, _P, _P], ct.c_int),
    "vh_zone_split": ([_P, _I64, _P], ct.c_int),
    "vh_batch_zones": ([_P, _P, ct.c_int32, _P, ct.c_int, ct.c_int, ct.c_int, ct.c_int32, ct.c_float], ct.c_int),
    "vh_batch_download_zones": ([_P, _P, _P, _P, _P, _P], ct.c_int),
    "vh_zones": ([_P, _P, _P, _P, _I64, _I64, _I64, _I64, ct.c_float, _P, ct.c_int32, _P, ct.c_int, ct.c_int,
                  ct.c_int, ct.c_int32, ct.c_float, _P, _P, _P, _P, _P], ct.c_int),
    "vh_batch_noise_sigma": ([_P, _P], ct.c_int),
    "vh_batch_denoise": ([_P, _P, ct.c_float, ct.c_int, ct.c_int, ct.c_int], ct.c_int),
    "vh_batch_download_hp": ([_P, _P], ct.c_int),
    "vh_noise_sigma": ([_P, _P, _P, _I64, _I64, _I64, _I64, _P], ct.c_int),
    "vh_denoise": ([_P, _P, _I64, _I64, _I64, _I64, _P, ct.c_float, ct.c_int, ct.c_int, ct.c_int, _P], ct.c_int),
    "vh_batch_edit_mask": ([_P, ct.c_int, _P], ct.c_int),
    "vh_batch_paint_mask": ([_P, _P, ct.c_int], ct.c_int),
    "vh_batch_download_mask": ([_P, _P, _P], ct.c_int),
    "vh_edit_mask": ([_P, _P, _I64, _I64, _I64, _I64, ct.c_int, _P, _P, _P], ct.c_int),
    "vh_batch_upload_proton": ([_P, _P], ct.c_int),
    "vh_batch_proton_threshold": ([_P, _P, _P, _P], ct.c_int),
    "vh_otsu": ([_P, ct.c_int32, _P], ct.c_int),
    "vh_batch_segment": ([_P, _P, _P], ct.c_int),
    "vh_batch_mask_overlap": ([_P, _P, _P], ct.c_int),
    "vh_segment": ([_P, _P, _I64, _I64, _I64, _I64, _P, _P, _P, _P, _P], ct.c_int),
    "vh_batch_register": ([_P, _P, _P, _P, _P, _P], ct.c_int),
    "vh_batch_download_register_hist": ([_P, _P], ct.c_int),
    "vh_mi": ([_P, ct.c_int32, ct.POINTER(ct.c_double)], ct.c_int),
    "vh_register_pick": ([_P, _P, _P], ct.c_int),
    "vh_batch_shift": ([_P, ct.c_int, _P], ct.c_int),
    "vh_batch_download_proton": ([_P, _P], ct.c_int),
    "vh_register": ([_P, _P, _P, _I64, _I64, _I64, _I64, _P, _P, _P, _P, _P], ct.c_int),
    "vh_resample_taps": ([_I64, _I64, ct.c_double, ct.c_double, _P, _P, _P], ct.c_int),
    "vh_batch_upload_proton_src": ([_P, _P, _P], ct.c_int),
    "vh_batch_resample_proton": ([_P, _P], ct.c_int),
    "vh_batch_download_proton_src": ([_P, _P], ct.c_int),
    "vh_resample": ([_P, _P, _P, _I64, _I64, _I64, _I64, _P, _P], ct.c_int),
    "vh_batch_register_maps": ([_P, _P, _P, _P, _P, _P, _P, _P, _P], ct.c_int),
    "vh_batch_download_register_maps_hist": ([_P, _P], ct.c_int),
    "vh_register_maps_pick": ([_P, _P, _P, _P], ct.c_int),
    "vh_axis_candidates": ([ct.c_double, ct.c_double, _I64, _P, ct.c_int32, _P, ct.c_int32, _P], ct.c_int),
    "vh_register_maps": ([_P, _P, _P, _P, _I64, _I64, _I64, _I64, _P, _P, _P, _P, _P, _P, _P], ct.c_int),
    "vh_recon": ([_P, _P, _I64, _I64, _I64, _P], ct.c_int),
    "vh_pipe_create": ([_P, _I64, _I64, _I64, _I64, ct.c_int, ct.POINTER(_P)], ct.c_int),
    "vh_pipe_run": ([_P, _P, _P, _I64, ct.POINTER(RunOpts), _P, _P, _P, _P, _P], ct.c_int),
    "vh_pipe_destroy": ([_P], ct.c_int),
    "vh_pipe_stats": ([_P, ct.POINTER(ct.c_int64), ct.POINTER(ct.c_int64)], ct.c_int),
    "vh_link_probe": ([_P, ct.c_int64, ct.POINTER(ct.c_double)], ct.c_int),
    "vh_host_alloc": ([_P, ct.c_int64, ct.POINTER(_P)], ct.c_int),
    "vh_host_free": ([_P], ct.c_int),
    "vh_comm_unique_id": ([_P], ct.c_int),
    "vh_comm_init": ([_P, ct.c_int, ct.c_int, _P], ct.c_int),
    "vh_batch_cohort_allreduce": ([_P], ct.c_int),
    "vh_comm_info": ([_P, ct.POINTER(ct.c_int), ct.POINTER(ct.c_int)], ct.c_int),
    "vh_comm_destroy": ([_P], ct.c_int),
}
EXPORTED = tuple(_SIGS)
ABI_VERSION = 8   # include/vent_hip.h VH_ABI_VERSION

_lib = None
_lock = threading.RLock()


def lib():
    """Load libventhip.so; fails loudly when the HIP extension has not been built."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise ImportError(f"{LIB_PATH} is missing: build it with "
                                      "`python __graft_entry__.py build` (no CPU fallback exists)")
                L = ct.CDLL(LIB_PATH)
                for name, (args, res) in _SIGS.items():
                    f = getattr(L, name)
                    f.argtypes = args
                    f.restype = res
                v = L.vh_abi_version()
                if v != ABI_VERSION:   # a stale build: its structs and signatures differ
                    raise ImportError(f"{LIB_PATH} has ABI version {v}, this shim needs "
                                      f"{ABI_VERSION}: rebuild it (`python __graft_entry__.py build`)")
                _lib = L
    return _lib


def empty_aligned(shape, dtype, align=4096):
    """np.empty whose data starts on a page boundary.  vh_pipe DMAs caller arrays in place, chunk
    by chunk; when every chunk boundary is page aligned (a study is 384 pages at 128x128x24 float32)
    no chunk needs the sub-page head / tail copies through staging, which run as blit kernels that
    wait for a free CU behind the N4 kernel."""
    dtype = np.dtype(dtype)
    n = int(np.prod(shape)) * dtype.itemsize
    buf = np.empty(n + align, np.uint8)
    off = (-buf.ctypes.data) % align
    return buf[off:off + n].view(dtype).reshape(shape)


def _ptr(a):
    return None if a is None else ct.c_void_p(a.ctypes.data)


class _PinnedPool:
    """Page-locked host buffers (vh_host_alloc) for the arrays an entry point returns: their D2H
    runs at the link rate with no runtime staging.  A returned array's buffer goes back to the pool
    when the last view of it is gone (a finalizer on the ctypes buffer numpy holds as its base); the
    pool keeps at most ``keep`` idle buffers per size.  r4: the CI line's dense f64 map."""

    def __init__(self, ctx, keep=4):
        self.ctx = ctx
        self.keep = keep
        self.idle = {}
        self.lock = threading.Lock()

    def array(self, shape, dtype):
        dtype = np.dtype(dtype)
        n = int(np.prod(shape)) * dtype.itemsize
        with self.lock:
            ptrs = self.idle.get(n)
            ptr = ptrs.pop() if ptrs else None
        if ptr is None:
            h = _P()
            self.ctx.check(self.ctx.L.vh_host_alloc(self.ctx.h, n, ct.byref(h)), "vh_host_alloc")
            ptr = h.value
        buf = (ct.c_char * n).from_address(ptr)
        weakref.finalize(buf, self._release, n, ptr)
        return np.frombuffer(buf, dtype).reshape(shape)

    def _release(self, n, ptr):
        with self.lock:
            ptrs = self.idle.setdefault(n, [])
            if self.ctx.h is not None and len(ptrs) < self.keep:
                ptrs.append(ptr)
                return
        lib().vh_host_free(ct.c_void_p(ptr))

    def close(self):
        with self.lock:
            for ptrs in self.idle.values():
                for p in ptrs:
                    lib().vh_host_free(ct.c_void_p(p))
            self.idle.clear()


class Context:
    """One device + one HIP stream (vh_ctx)."""

    def __init__(self, device: int = 0):
        self.L = lib()
        h = _P()
        rc = self.L.vh_create(int(device), ct.byref(h))
        if rc != VH_OK:
            raise VentHipError(f"vh_create(device={device}) failed: "
                               f"{self.L.vh_status_string(rc).decode()}")
        self.h = h
        self.device = device
        # (table key, R, C) -> (table, vh_ci_table handle), least recently used first: tables stay
        # in HBM.  ci_lock covers the lookup, any eviction and the vh_ci_tab call that uses the
        # handle, so no thread's handle is destroyed under it
        self.ci_tables = {}
        self.ci_lock = threading.RLock()
        self.pinned = _PinnedPool(self)

    def link_probe(self, nbytes=256 << 20):
        """PCIe rates of this context's GPU with pinned host memory, GB/s: H2D alone, D2H alone,
        both at once on two streams (vh_link_probe)."""
        out = (ct.c_double * 3)()
        self.check(self.L.vh_link_probe(self.h, int(nbytes), out), "vh_link_probe")
        return {"h2d_GBps": round(out[0], 2), "d2h_GBps": round(out[1], 2), "both_GBps": round(out[2], 2)}

    CI_TABLES_KEPT = 16

    def ci_table(self, table, R, C):
        """The device copy of a compact sphere table for (R, C) volumes (vh_ci_table_create, once
        per table content; the reference caches the table file the same way, CI.py:43-61).  Keyed
        by ``table.key`` -- (vox, Rmax, R, C) for sphere.compact_table_for's tables -- or by the
        object for ad-hoc tables.  Call with ``ci_lock`` held for as long as the handle is used."""
        tk = getattr(table, "key", None)
        key = (tk if tk is not None else ("obj", id(table)), int(R), int(C))
        hit = self.ci_tables.pop(key, None)
        if hit is not None and (tk is not None or hit[0] is table):
            self.ci_tables[key] = hit   # most recently used last
            return hit[1]
        if hit is not None:   # an ad-hoc table whose id was reused
            self.L.vh_ci_table_destroy(hit[1])
        while len(self.ci_tables) >= self.CI_TABLES_KEPT:   # drop the least recently used
            k0 = next(iter(self.ci_tables))
            self.L.vh_ci_table_destroy(self.ci_tables.pop(k0)[1])   # locks ctx->mu, drains
        h = _P()
        self.check(self.L.vh_ci_table_create(self.h, int(R), int(C), _ptr(table.offsets),
                                             _ptr(table.dup), table.rows, _ptr(table.bounds),
                                             _ptr(table.radii), table.bounds.shape[0], ct.byref(h)),
                   "vh_ci_table_create")
        self.ci_tables[key] = (table, h)
        return h

    def close(self):
        if getattr(self, "h", None):
            self.pinned.close()
            with self.ci_lock:
                for _, th in self.ci_tables.values():
                    self.L.vh_ci_table_destroy(th)
                self.ci_tables.clear()
            self.L.vh_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc: int, where: str):
        if rc == VH_OK:
            return
        msg = (self.L.vh_last_error(self.h) or b"").decode() if self.h else ""
        text = f"{where}: {self.L.vh_status_string(rc).decode()}: {msg}"
        if rc == VH_ERR_MAXRADIUS:
            raise ValueError(text)
        if rc in (VH_ERR_EMPTY, VH_ERR_INDEX):
            raise IndexError(text)
        if rc == VH_ERR_ARG:
            raise ValueError(text)
        if rc == VH_ERR_NOMEM:
            raise MemoryError(text)
        raise VentHipError(text)


_ctx = {}
_live = weakref.WeakSet()   # open Batch / Pipe objects


@atexit.register
def _shutdown():
    """Destroy the cached contexts (their scratch batches, streams and device buffers) while the HIP
    runtime -- and a profiler attached to it -- is still fully up.  Left to interpreter teardown,
    vh_destroy ran in no defined order, possibly after C-level exit handlers had started taking the
    runtime and rocprofv3 down (SIGSEGV in exit() after profiled cooperative launches)."""
    with _lock:
        _batch_pool.clear()
        for o in list(_live):   # batches and pipes first: they hold their context
            try:
                o.close()
            except Exception:
                pass
        for c in list(_ctx.values()):
            try:
                c.close()
            except Exception:
                pass
        _ctx.clear()


def context(device: int = 0) -> Context:
    c = _ctx.get(device)
    if c is None:
        with _lock:
            c = _ctx.get(device)
            if c is None:
                c = Context(device)
                _ctx[device] = c
    return c


def device_count() -> int:
    n = ct.c_int(0)
    lib().vh_device_count(ct.byref(n))
    return n.value


def n4_params(max_iters=(50, 50, 50, 50), conv_threshold=0.001, ncp=(4, 4, 4), n_bins=200,
              wiener_noise=0.01, fwhm=0.15, conv_mode=0) -> N4Params:
    """SimpleITK N4BiasFieldCorrectionImageFilter defaults (Vent_Analysis.py:330).  conv_mode 0 is
    ITK's float Welford convergence measure (reference iteration counts); 1 the exact CoV."""
    p = N4Params()
    lib().vh_n4_default_params(ct.byref(p))
    p.n_levels = len(max_iters)
    for i in range(8):
        p.max_iters[i] = max_iters[i] if i < len(max_iters) else 0
    p.conv_threshold = conv_threshold
    for i in range(3):
        p.ncp[i] = ncp[i]
    p.n_bins = n_bins
    p.wiener_noise = wiener_noise
    p.fwhm = fwhm
    p.conv_mode = int(conv_mode)
    return p


def as_batch(a, dtype):
    """(R,C,Z) or (B,R,C,Z) -> contiguous (B,R,C,Z) of dtype (DICOM arrays are transposed views,
    Vent_Analysis.py:179, so a contiguous copy is made when needed)."""
    a = np.asarray(a)
    if a.ndim == 3:
        a = a[None]
    if a.ndim != 4:
        raise ValueError(f"expected a 3-D volume or a 4-D batch, got shape {a.shape}")
    return np.ascontiguousarray(a, dtype=dtype)


# ---- thin wrappers over the host-buffer entry points -------------------------------------------
def n4(hp, mask, device=0, **kw):
    c = context(device)
    h = as_batch(hp, np.float32)
    m = as_batch(mask, np.uint8)
    if h.shape != m.shape:
        raise ValueError("HPvent and mask shapes differ")
    B, R, C, Z = h.shape
    p = n4_params(**kw)
    out = np.empty_like(h)
    its = np.zeros((B, p.n_levels), np.int32)
    conv = np.zeros((B, p.n_levels), np.float32)
    c.check(c.L.vh_n4(c.h, _ptr(h), _ptr(m), R, C, Z, B, ct.byref(p), _ptr(out), _ptr(its),
                      _ptr(conv)), "vh_n4")
    return out, its, conv


def border(a, device=0):
    c = context(device)
    x = as_batch(a, np.uint8)
    B, R, C, Z = x.shape
    out = np.empty_like(x)
    c.check(c.L.vh_border(c.h, _ptr(x), R, C, Z, B, _ptr(out)), "vh_border")
    return out


def snr(hp, mask, device=0):
    c = context(device)
    h = as_batch(hp, np.float32)
    m = as_batch(mask, np.uint8)
    B, R, C, Z = h.shape
    out = np.zeros(B, np.float64)
    c.check(c.L.vh_snr(c.h, _ptr(h), _ptr(m), R, C, Z, B, _ptr(out)), "vh_snr")
    return out


def vdp(n4v, mask, vox, hp=None, thresh=0.6, device=0):
    c = context(device)
    n = as_batch(n4v, np.float32)
    m = as_batch(mask, np.uint8)
    h = None if hp is None else as_batch(hp, np.float32)
    B, R, C, Z = n.shape
    defect = np.empty((B, R, C, Z), np.uint8)
    bord = np.empty_like(defect)
    lb = np.empty_like(defect)
    res = (VdpResult * B)()
    vx = np.ascontiguousarray(vox, dtype=np.float64)
    c.check(c.L.vh_vdp(c.h, _ptr(h), _ptr(n), _ptr(m), R, C, Z, B, ct.c_float(thresh), _ptr(vx),
                       _ptr(defect), _ptr(bord), _ptr(lb), ct.cast(res, ct.c_void_p)), "vh_vdp")
    return defect, bord, lb, list(res)


def defect_map(n4, mask, source, medfilt=1, thresh=0.6, device=0, km=False):
    """The defect map of one thresholding from host arrays (vh_defect_map): ``source`` 'mean' | 'lb'
    | 'kmeans', ``medfilt`` 0 / 1 / 2 as Batch.select_defect.  Returns (defect, border, count), uint8
    [B][R][C][Z] twice and int64 [B], with the k-means label map appended when ``km``."""
    c = context(device)
    n = as_batch(n4, np.float32)
    m = as_batch(mask, np.uint8)
    if n.shape != m.shape:
        raise ValueError("N4 and mask shapes differ")
    B, R, C, Z = n.shape
    d = np.empty((B, R, C, Z), np.uint8)
    bo = np.empty_like(d)
    lab = np.empty_like(d) if km else None
    cnt = np.zeros(B, np.int64)
    c.check(c.L.vh_defect_map(c.h, _ptr(n), _ptr(m), R, C, Z, B, ct.c_float(thresh),
                              defect_source(source), int(medfilt), _ptr(d), _ptr(bo), _ptr(lab),
                              _ptr(cnt)), "vh_defect_map")
    return (d, bo, cnt, lab) if km else (d, bo, cnt)


def distribution(n4, mask, norm="p99", bins=1024, hi=1.5, thresh=0.6, device=0):
    """The ventilation distribution from host arrays (vh_distribution): the post-N4 chain, then per
    study the histogram of float32(N4 / d) over the mask (``norm`` 'mean' | 'p99' picks d) and the
    slice counts of the mask, the run's mean-anchored defect map and the six LB classes.  Returns the
    dict of Batch.download_distribution.  IndexError for an empty-mask study, like vdp()."""
    c = context(device)
    n = as_batch(n4, np.float32)
    m = as_batch(mask, np.uint8)
    if n.shape != m.shape:
        raise ValueError("N4 and mask shapes differ")
    B, R, C, Z = n.shape
    bins = int(bins)
    hist = np.zeros((B, max(bins, 0)), np.uint32)
    outside = np.zeros((B, 2), np.int64)
    sl = np.zeros((B, Z, VH_DIST_COLS), np.int64)
    c.check(c.L.vh_distribution(c.h, _ptr(n), _ptr(m), R, C, Z, B, ct.c_float(thresh), norm_source(norm),
                                bins, ct.c_float(hi), _ptr(hist), _ptr(outside), _ptr(sl)), "vh_distribution")
    return dict(hist=hist, outside=outside, slice_counts=sl, edges=dist_edges(bins, hi))


def _heterogeneity_args(radius, min_count, bins, hi):
    """The checked (radius, min_count, bins, hi) of vh_batch_heterogeneity; ``min_count`` None is the
    majority of the window, (2 radius + 1)^2 // 2 + 1.  ValueError for what the library would refuse,
    so the message names the argument."""
    def whole(v, what):
        if isinstance(v, (bool, float)) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"heterogeneity: {what} is an int, got {v!r}")
        return int(v)
    radius = whole(radius, "radius")
    if not 1 <= radius <= 5:
        raise ValueError(f"heterogeneity: radius must be 1..5, got {radius!r}")
    win = (2 * radius + 1) ** 2
    min_count = win // 2 + 1 if min_count is None else whole(min_count, "min_count")
    if not 2 <= min_count <= win:
        raise ValueError(f"heterogeneity: min_count must be 2..{win} at radius {radius}, got {min_count!r}")
    bins = whole(bins, "bins")
    if not 1 <= bins <= 1024:
        raise ValueError(f"heterogeneity: bins must be 1..1024, got {bins!r}")
    h = np.float32(hi)
    if not (np.isfinite(h) and 0 < h <= 16):
        raise ValueError(f"heterogeneity: hi must be finite, > 0 and <= 16, got {hi!r}")
    return radius, min_count, bins, float(h)


def het_index(stats):
    """The ventilation heterogeneity index of each study from its ``stats`` row(s) (n_in, n_over,
    n_none, sum_fx): float64 sum_fx / 2^24 / n_in, the mean CoV over the in-range voxels; NaN where
    n_in == 0."""
    st = np.asarray(stats, dtype=np.int64)
    n_in = st[..., 0].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(n_in > 0, st[..., 3].astype(np.float64) / 16777216.0 / n_in, np.nan)


def heterogeneity(x, mask, radius=1, min_count=None, bins=100, hi=1.0, device=0):
    """The local ventilation heterogeneity from host arrays (vh_heterogeneity; the spec is in
    include/vent_hip.h): ``x`` a 3-D volume or a 4-D batch, ``mask`` of the same shape and any dtype,
    nonzero counting as set.  No run and no N4 behind it; to exclude defects, AND them out of the mask.
    Returns the dict of Batch.download_heterogeneity."""
    c = context(device)
    v = as_batch(x, np.float32)
    m = as_batch(_mask_u8(mask), np.uint8)
    if v.shape != m.shape:
        raise ValueError("volume and mask shapes differ")
    radius, min_count, bins, hi = _heterogeneity_args(radius, min_count, bins, hi)
    B, R, C, Z = v.shape
    out = np.empty_like(v)
    hist = np.zeros((B, bins), np.uint32)
    stats = np.zeros((B, 4), np.int64)
    c.check(c.L.vh_heterogeneity(c.h, _ptr(v), _ptr(m), R, C, Z, B, radius, min_count, bins, ct.c_float(hi),
                                 _ptr(out), _ptr(hist), _ptr(stats)), "vh_heterogeneity")
    return dict(map=out, hist=hist, edges=dist_edges(bins, hi), stats=stats, index=het_index(stats))


def depth_thresholds(edges):
    """Band edges in pixels (floats allowed), increasing -> the uint16 thresholds ceil(e * e) of
    vh_batch_core_rind, computed in double: a voxel is at least e pixels deep, D2 >= e^2, exactly when
    D2 >= ceil(e^2), D2 being an integer.  ValueError for an edge that is not finite or not > 0, for a
    threshold above 65535, for thresholds that are not strictly increasing (two edges with one
    threshold included) and for more than 31 edges."""
    e = np.atleast_1d(np.asarray(edges, dtype=np.float64)) if np.size(edges) else np.zeros(0, np.float64)
    if e.ndim != 1:
        raise ValueError(f"core_rind: edges is a sequence of numbers, got shape {e.shape}")
    if e.size > 31:
        raise ValueError(f"core_rind: at most 31 edges, got {e.size}")
    if not (np.isfinite(e).all() and (e > 0).all()):
        raise ValueError(f"core_rind: every edge must be finite and > 0, got {edges!r}")
    t = np.ceil(e * e)
    if (t > 65535).any():
        raise ValueError(f"core_rind: an edge's threshold ceil(e^2) exceeds 65535, got {edges!r}")
    if (np.diff(t) <= 0).any():
        raise ValueError(f"core_rind: the edges must give strictly increasing thresholds, got {t.astype(int).tolist()}")
    return t.astype(np.uint16)


def _core_rind_args(edges, thresholds):
    """The uint16 thresholds of vh_batch_core_rind: depth_thresholds(edges), or ``thresholds`` (ints,
    1 <= t[0] < t[1] < ... <= 65535, at most 31) as they are when given.  ValueError for what the
    library would refuse, so the message names the argument."""
    if thresholds is None:
        return depth_thresholds(edges)
    t = np.asarray(thresholds)
    if t.size == 0:
        return np.zeros(0, np.uint16)
    if t.ndim != 1 or t.dtype == np.bool_ or not np.issubdtype(t.dtype, np.integer):
        raise ValueError(f"core_rind: thresholds is a sequence of ints, got {thresholds!r}")
    if t.size > 31:
        raise ValueError(f"core_rind: at most 31 thresholds, got {t.size}")
    t = t.astype(np.int64)
    if t[0] < 1 or t[-1] > 65535 or (np.diff(t) <= 0).any():
        raise ValueError(f"core_rind: thresholds must be strictly increasing in 1..65535, got {t.tolist()}")
    return t.astype(np.uint16)


def band_vdp(counts):
    """float64 100 * defect / mask of each band from ``counts`` [...][2]; NaN for an empty band."""
    c = np.asarray(counts, dtype=np.int64)
    n = c[..., 0].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(n > 0, 100.0 * c[..., 1].astype(np.float64) / n, np.nan)


def core_rind_form(R, C, Z):
    """'rows' or 'global': which form of the search a study shape takes (vh_core_rind_form; no device)."""
    f = lib().vh_core_rind_form(int(R), int(C), int(Z))
    if f not in (0, 1):
        raise ValueError(f"core_rind_form: dims must be >= 1, got {(R, C, Z)!r}")
    return ("rows", "global")[f]


def core_rind(mask, defect=None, edges=(1.5, 3.5), device=0, thresholds=None):
    """The core-rind analysis from host arrays (vh_core_rind; the spec is in include/vent_hip.h):
    ``mask`` a 3-D volume or a 4-D batch of any dtype, nonzero counting as set; ``defect`` of the same
    shape, or None for a defect column of 0.  No run behind it.  Returns the dict of
    Batch.download_core_rind."""
    thr = _core_rind_args(edges, thresholds)
    m = as_batch(_mask_u8(mask), np.uint8)
    d = None if defect is None else as_batch(_mask_u8(defect), np.uint8)
    if d is not None and d.shape != m.shape:
        raise ValueError("mask and defect shapes differ")
    c = context(device)
    B = m.shape[0]
    out = np.empty(m.shape, np.uint16)
    counts = np.zeros((B, thr.size + 1, 2), np.int64)
    stats = np.zeros((B, 2), np.int64)
    c.check(c.L.vh_core_rind(c.h, _ptr(m), _ptr(d), *m.shape[1:], B, _ptr(thr), thr.size,
                             _ptr(out), _ptr(counts), _ptr(stats)), "vh_core_rind")
    return dict(d2=out, counts=counts, stats=stats, thresholds=thr, band_vdp=band_vdp(counts))


VH_ZONE_EXTENT, VH_ZONE_COUNT = range(2)   # vh_batch_zones: how an axis is cut into parts
VH_ZONE_COLS = 8                           # counts columns: mask, defect (on the mask), LB class 1..6
_ZONE_BYS = {"extent": VH_ZONE_EXTENT, "count": VH_ZONE_COUNT}
ZONE_MAX = 32                              # the most zones, and the most parts of an axis


def zone_by(by) -> int:
    """'extent' | 'count' or the VH_ZONE_* ints -> the int; anything else raises ValueError."""
    return _named_int(by, _ZONE_BYS, "zones: by")


def _zones_args(parts=(3, 1, 1), lateral=True, by="extent", labels=None, n_zones=None, norm="mean", bins=100,
                hi=1.5, shape=None):
    """The checked arguments of vh_batch_zones as a dict: ``labels`` (uint8, contiguous, of ``shape``
    when given, or None), ``n_zones``, ``parts`` int32 [3], ``lateral``, ``by``, ``norm``, ``bins``,
    ``hi`` and ``K``, the zones without zone 0.  With ``labels`` the geometric arguments are not looked
    at and ``n_zones`` None is the largest label.  ValueError for what the library would refuse, so the
    message names the argument."""
    def whole(v, what):
        if isinstance(v, (bool, float)) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"zones: {what} is an int, got {v!r}")
        return int(v)
    norm = norm_source(norm)
    if norm not in (VH_NORM_MEAN, VH_NORM_P99):
        raise ValueError(f"zones: norm is 'mean' or 'p99' or 0..1, got {norm!r}")
    bins = whole(bins, "bins")
    if not 1 <= bins <= 256:
        raise ValueError(f"zones: bins must be 1..256, got {bins!r}")
    h = np.float32(hi)
    if not (np.isfinite(h) and 0 < h <= 64):
        raise ValueError(f"zones: hi must be finite, > 0 and <= 64, got {hi!r}")
    out = dict(labels=None, n_zones=0, parts=np.ones(3, np.int32), lateral=0, by=VH_ZONE_EXTENT, norm=norm,
               bins=bins, hi=float(h))
    if labels is not None:
        lab = np.asarray(labels)
        if lab.dtype == np.bool_ or not np.issubdtype(lab.dtype, np.integer):
            raise ValueError(f"zones: labels is an integer volume, got dtype {lab.dtype}")
        if shape is not None and lab.shape != tuple(shape):
            raise ValueError(f"zones: labels must have shape {tuple(shape)}, got {lab.shape}")
        if lab.dtype != np.uint8:   # (a label outside a byte is no zone: 0, like every byte above K)
            lab = np.where((lab >= 0) & (lab <= 255), lab, 0)
        n_zones = int(lab.max()) if n_zones is None and lab.size else whole(0 if n_zones is None else n_zones, "n_zones")
        if not 1 <= n_zones <= ZONE_MAX:
            raise ValueError(f"zones: n_zones must be 1..{ZONE_MAX}, got {n_zones!r}")
        out.update(labels=np.ascontiguousarray(lab, dtype=np.uint8), n_zones=n_zones, K=n_zones)
        return out
    by = zone_by(by)
    if isinstance(lateral, (float, str)) or lateral not in (0, 1, False, True):
        raise ValueError(f"zones: lateral is a bool, got {lateral!r}")
    lateral = int(lateral)
    p = np.asarray(parts)
    if p.shape != (3,) or p.dtype == np.bool_ or not np.issubdtype(p.dtype, np.integer):
        raise ValueError(f"zones: parts is three ints (rows, columns, slices), got {parts!r}")
    p = p.astype(np.int64)
    if (p < 1).any():
        raise ValueError(f"zones: every part count must be >= 1, got {parts!r}")
    if lateral and p[1] != 1:
        raise ValueError(f"zones: lateral takes the column axis, parts[1] must be 1, got {parts!r}")
    K = int(p[0] * (2 if lateral else p[1]) * p[2])
    if K > ZONE_MAX:
        raise ValueError(f"zones: at most {ZONE_MAX} zones, got {K} from parts {parts!r}"
                         + (" with lateral" if lateral else ""))
    out.update(parts=np.ascontiguousarray(p, dtype=np.int32), lateral=lateral, by=by, K=K)
    return out


def zone_vdp(counts):
    """float64 100 * defect / mask of each zone from ``counts`` [...][8]; NaN for an empty zone."""
    return band_vdp(np.asarray(counts, dtype=np.int64)[..., :2])


def zone_mean(stats):
    """The mean normalised signal of each zone from its ``stats`` row(s) (n_in, n_below, n_over,
    sum_fx): float64 sum_fx / 2^24 / n_in over the in-range voxels; NaN where n_in == 0."""
    return het_index(stats)


def _zones_dict(a, m, c, h, s, g):
    return dict(map=m, counts=c, hist=h, edges=dist_edges(a["bins"], a["hi"]), stats=s, geom=g,
                zone_vdp=zone_vdp(c), zone_mean=zone_mean(s), n_zones=a["K"])


def zone_parts(profile, p, by="extent"):
    """The parts of one axis from its mask profile (vh_zone_parts; no device): (part uint8 [n],
    (lo, hi)).  ``profile`` holds the on voxels of every plane of the axis, ints >= 0."""
    prof = np.ascontiguousarray(profile, dtype=np.int64)
    if prof.ndim != 1 or prof.size < 1:
        raise ValueError(f"zone_parts: profile is a non-empty sequence of ints, got shape {prof.shape}")
    if isinstance(p, (bool, float)) or not isinstance(p, (int, np.integer)) or not 1 <= int(p) <= ZONE_MAX:
        raise ValueError(f"zone_parts: p must be 1..{ZONE_MAX}, got {p!r}")
    part = np.zeros(prof.size, np.uint8)
    bounds = np.zeros(2, np.int32)
    if lib().vh_zone_parts(_ptr(prof), prof.size, int(p), zone_by(by), _ptr(part), _ptr(bounds)) != VH_OK:
        raise ValueError("zone_parts: the profile holds a negative entry or its total exceeds 2^57")
    return part, (int(bounds[0]), int(bounds[1]))


def zone_split(profile):
    """The lateral split column of a column profile (vh_zone_split; no device)."""
    prof = np.ascontiguousarray(profile, dtype=np.int64)
    if prof.ndim != 1 or prof.size < 1:
        raise ValueError(f"zone_split: profile is a non-empty sequence of ints, got shape {prof.shape}")
    s = ct.c_int32(0)
    if lib().vh_zone_split(_ptr(prof), prof.size, ct.byref(s)) != VH_OK:
        raise ValueError("zone_split: the profile holds a negative entry or its total exceeds 2^57")
    return int(s.value)


def zones(n4, mask, defect=None, parts=(3, 1, 1), lateral=True, by="extent", labels=None, n_zones=None,
          norm="mean", bins=100, hi=1.5, thresh=0.6, device=0, map=True):
    """The regional analysis from host arrays (vh_zones; the spec is in include/vent_hip.h): the
    post-N4 chain on ``n4`` and ``mask`` (3-D volumes or 4-D batches), ``defect`` (None: the chain's
    mean-anchored map at ``thresh``) as the defect map, then the zones.  Returns the dict of
    Batch.download_zones.  IndexError for an empty-mask study, like vdp()."""
    c = context(device)
    n = as_batch(n4, np.float32)
    m = as_batch(_mask_u8(mask), np.uint8)
    d = None if defect is None else as_batch(_mask_u8(defect), np.uint8)
    if n.shape != m.shape or (d is not None and d.shape != m.shape):
        raise ValueError("N4, mask and defect shapes differ")
    if labels is not None and np.ndim(labels) == 3:
        labels = np.asarray(labels)[None]
    a = _zones_args(parts, lateral, by, labels, n_zones, norm, bins, hi, n.shape)
    B, R, C, Z = n.shape
    K1 = a["K"] + 1
    out = np.empty(n.shape, np.uint8) if map else None
    counts = np.zeros((B, K1, VH_ZONE_COLS), np.int64)
    hist = np.zeros((B, K1, a["bins"]), np.uint32)
    stats = np.zeros((B, K1, 4), np.int64)
    geom = np.zeros((B, 8), np.int32)
    c.check(c.L.vh_zones(c.h, _ptr(n), _ptr(m), _ptr(d), R, C, Z, B, ct.c_float(thresh), _ptr(a["labels"]),
                         a["n_zones"], _ptr(a["parts"]), a["lateral"], a["by"], a["norm"], a["bins"],
                         ct.c_float(a["hi"]), _ptr(out), _ptr(counts), _ptr(hist), _ptr(stats), _ptr(geom)),
            "vh_zones")
    return _zones_dict(a, out, counts, hist, stats, geom)


VH_CC_DEFECT, VH_CC_MASK = range(2)     # vh_batch_components sources
_CC_SOURCES = {"defect": VH_CC_DEFECT, "mask": VH_CC_MASK}
CC_CONNS = (4, 8, 6, 26)


def _cc_conn(conn):
    """4 | 8 (per slice) | 6 | 26 -> the int; anything else raises ValueError."""
    if isinstance(conn, (bool, float)) or not isinstance(conn, (int, np.integer)) or int(conn) not in CC_CONNS:
        raise ValueError(f"components: conn is one of 4, 8, 6, 26, got {conn!r}")
    return int(conn)


def _components_args(source, conn, edges):
    """(source int, conn int, edges uint32 contiguous) for vh_batch_components: ``source`` 'defect' |
    'mask' or the VH_CC_* ints; ``conn`` 4 | 8 | 6 | 26; ``edges`` at most 31 ints, 2 <= e[0] < e[1] <
    ... < 2^32.  ValueError for what the library would refuse, so the message names the argument."""
    source = _named_int(source, _CC_SOURCES, "components source")
    conn = _cc_conn(conn)
    e = np.asarray(edges)
    if e.size == 0:
        return source, conn, np.zeros(0, np.uint32)
    if e.ndim != 1 or e.dtype == np.bool_ or not np.issubdtype(e.dtype, np.integer):
        raise ValueError(f"components: edges is a sequence of ints, got {edges!r}")
    if e.size > 31:
        raise ValueError(f"components: at most 31 edges, got {e.size}")
    e = e.astype(np.int64) if e.dtype != np.uint64 else e
    if e[0] < 2 or e[-1] >= 2 ** 32 or (np.diff(e.astype(np.float64)) <= 0).any():
        raise ValueError(f"components: edges must be strictly increasing in 2..2^32 - 1, got {e.tolist()}")
    return source, conn, np.ascontiguousarray(e, dtype=np.uint32)


def _per_study_ints(v, n, lo, hi, dtype, what):
    """A scalar or one int per study -> ``dtype`` [n] contiguous, every value in lo..hi; else ValueError."""
    a = np.asarray(v)
    if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"filter_components: {what} is an int or one int per study, got {v!r}")
    if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != n):
        raise ValueError(f"filter_components: {n} studies, got {what} of shape {a.shape}")
    if a.size and (int(a.min()) < lo or int(a.max()) > hi):
        raise ValueError(f"filter_components: every {what} must be {lo}..{hi}, got {v!r}")
    return np.ascontiguousarray(np.broadcast_to(a, (n,)), dtype=dtype)


def _filter_components_args(source, conn, min_size, keep_largest, n):
    """(source int, conn int, min_size uint32 [n], keep_largest int32 [n]) for
    vh_batch_filter_components: ``min_size`` >= 1 and ``keep_largest`` 0..8 (0: no limit), each a scalar
    or one int per study.  ValueError for what the library would refuse."""
    source = _named_int(source, _CC_SOURCES, "components source")
    conn = _cc_conn(conn)
    return (source, conn, _per_study_ints(min_size, n, 1, 2 ** 32 - 1, np.uint32, "min_size"),
            _per_study_ints(keep_largest, n, 0, 8, np.int32, "keep_largest"))


def components(a, conn=6, edges=(), device=0):
    """The connected components of byte volumes on the host (vh_components; the spec is in
    include/vent_hip.h): ``a`` a 3-D volume or a 4-D batch of any dtype, nonzero counting as set.  No
    run behind it.  Returns the dict of Batch.download_components."""
    _, conn, e = _components_args(VH_CC_MASK, conn, edges)
    m = as_batch(_mask_u8(a), np.uint8)
    c = context(device)
    B = m.shape[0]
    root = np.empty(m.shape, np.int32)
    size = np.empty(m.shape, np.uint32)
    counts = np.zeros((B, e.size + 1, 2), np.int64)
    stats = np.zeros((B, 4), np.int64)
    c.check(c.L.vh_components(c.h, _ptr(m), *m.shape[1:], B, conn, _ptr(e), e.size, _ptr(root), _ptr(size),
                              _ptr(counts), _ptr(stats)), "vh_components")
    return dict(root=root, size=size, counts=counts, stats=stats, edges=e)


def filter_components(a, conn=6, min_size=1, keep_largest=0, device=0):
    """The component filter on the host (vh_filter_components): ``a`` as for components(); a component
    stays when it has ``min_size`` voxels and, with ``keep_largest`` = k > 0, is among the k largest
    (ties: the smaller root first); each a scalar or one int per study.  Returns (out, kept): uint8
    [B][R][C][Z], the kept voxels with their byte values (1 where ``a`` is not uint8), and int64 [B][2]
    = components kept, voxels kept."""
    m = as_batch(_mask_u8(a), np.uint8)
    B = m.shape[0]
    _, conn, ms, kl = _filter_components_args(VH_CC_MASK, conn, min_size, keep_largest, B)
    c = context(device)
    out = np.empty_like(m)
    kept = np.zeros((B, 2), np.int64)
    c.check(c.L.vh_filter_components(c.h, _ptr(m), *m.shape[1:], B, conn, _ptr(ms), _ptr(kl), _ptr(out),
                                     _ptr(kept)), "vh_filter_components")
    return out, kept


VH_DT_COLS, VH_DT_MAX_ROWS, VH_DT_NO_SIGNAL = 18, 1024, -1   # vh_batch_defect_table
DT_COLUMNS = ("root", "size", "sum_r", "sum_c", "sum_z", "min_r", "max_r", "min_c", "max_c", "min_z", "max_z",
              "faces_r", "faces_c", "faces_z", "n_sig", "sum_fx", "min_fx", "max_fx")


def _defect_table_args(min_size, max_rows, norm, n):
    """(min_size uint32 [n], max_rows int, norm int) for vh_batch_defect_table: ``min_size`` >= 1, a
    scalar or one int per study; ``max_rows`` 1..1024; ``norm`` None (no signal columns) | 'mean' |
    'p99'.  ValueError for what the library would refuse, so the message names the argument."""
    ms = _per_study_ints(min_size, n, 1, 2 ** 32 - 1, np.uint32, "min_size")
    if (isinstance(max_rows, (bool, float)) or not isinstance(max_rows, (int, np.integer))
            or not 1 <= int(max_rows) <= VH_DT_MAX_ROWS):
        raise ValueError(f"defect_table: max_rows must be an int in 1..{VH_DT_MAX_ROWS}, got {max_rows!r}")
    if norm is not None and not (isinstance(norm, str) and norm in _NORM_SOURCES):
        raise ValueError(f"defect_table: norm is None, 'mean' or 'p99', got {norm!r}")
    return ms, int(max_rows), VH_DT_NO_SIGNAL if norm is None else _NORM_SOURCES[norm]


def table_metrics(rows, vox):
    """What a reader wants of defect-table rows, in float64 from their integers alone: ``rows`` int64
    [...][18], ``vox`` the voxel edges (mm) along rows, columns and slices.  A dict of arrays over the
    leading axes, NaN for an unused row (column 0 = -1): ``volume_mL`` size * prod(vox / 10);
    ``centroid`` [...][3] the index sums / size, in voxels, and ``centroid_mm`` = centroid * vox;
    ``extent`` [...][3] max - min + 1 per axis; ``surface_mm2`` the voxel-face surface faces_r vox_c
    vox_z + faces_c vox_r vox_z + faces_z vox_r vox_c; ``sphericity`` pi^(1/3) (6 volume_mm3)^(2/3) /
    surface_mm2; ``mean``, ``min``, ``max`` of the normalised signal, sum_fx / 2^24 / n_sig, min_fx /
    2^24, max_fx / 2^24, NaN where n_sig = 0."""
    r = np.asarray(rows, dtype=np.int64)
    if r.shape[-1:] != (VH_DT_COLS,):
        raise ValueError(f"table_metrics: rows is [...][{VH_DT_COLS}], got shape {r.shape}")
    v = np.asarray(vox, dtype=np.float64)
    if v.shape != (3,):
        raise ValueError(f"table_metrics: vox is three edges (mm), got {vox!r}")
    f = r.astype(np.float64)
    used = r[..., 0] >= 0
    size = np.where(used, f[..., 1], np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        centroid = f[..., 2:5] / size[..., None]
        extent = np.where(used[..., None], f[..., 6:11:2] - f[..., 5:10:2] + 1.0, np.nan)
        surface = np.where(used, f[..., 11] * v[1] * v[2] + f[..., 12] * v[0] * v[2] + f[..., 13] * v[0] * v[1], np.nan)
        sphericity = np.pi ** (1.0 / 3.0) * (6.0 * size * np.prod(v)) ** (2.0 / 3.0) / surface
        n_sig = np.where(used & (r[..., 14] > 0), f[..., 14], np.nan)
        mean = f[..., 15] / 16777216.0 / n_sig
        lo = np.where(np.isnan(n_sig), np.nan, f[..., 16] / 16777216.0)
        hi = np.where(np.isnan(n_sig), np.nan, f[..., 17] / 16777216.0)
    return dict(volume_mL=size * np.prod(v / 10.0), centroid=centroid, centroid_mm=centroid * v, extent=extent,
                surface_mm2=surface, sphericity=sphericity, mean=mean, min=lo, max=hi)


def _denoise_args(sigma, n, strength, search, patch):
    """The per-study sigma as float32 [n] (a scalar is repeated) and the checked ints; ValueError for
    what the library would refuse, so the message names the argument."""
    sg = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma, dtype=np.float32), (n,)))
    if not (np.isfinite(sg).all() and (sg > 0).all()):
        raise ValueError(f"denoise: every sigma must be finite and > 0, got {sg}")
    if isinstance(search, (bool, float)) or isinstance(patch, (bool, float)):
        raise ValueError("denoise: search and patch are ints")
    if not 1 <= int(search) <= 5:
        raise ValueError(f"denoise: search must be 1..5, got {search!r}")
    if not 0 <= int(patch) <= 2:
        raise ValueError(f"denoise: patch must be 0..2, got {patch!r}")
    if not (np.isfinite(np.float32(strength)) and np.float32(strength) > 0):
        raise ValueError(f"denoise: strength must be finite and > 0, got {strength!r}")
    return sg, int(search), int(patch)


def noise_sigma(hp, mask, device=0):
    """The noise of each study from host arrays (vh_noise_sigma): float32 [B], sqrt(S2 / (2 N)) over
    the voxels calculate_SNR counts as noise (the Rayleigh maximum-likelihood estimate of a magnitude
    background); NaN where the SNR is undefined."""
    c = context(device)
    h = as_batch(hp, np.float32)
    m = as_batch(mask, np.uint8)
    if h.shape != m.shape:
        raise ValueError("HPvent and mask shapes differ")
    B, R, C, Z = h.shape
    out = np.zeros(B, np.float32)
    c.check(c.L.vh_noise_sigma(c.h, _ptr(h), _ptr(m), R, C, Z, B, _ptr(out)), "vh_noise_sigma")
    return out


def denoise(hp, sigma, strength=2.0, search=3, patch=1, rician=False, device=0):
    """The in-plane non-local-means filter from host arrays (vh_denoise; the spec is in
    include/vent_hip.h): ``sigma`` a scalar or one value per study.  Returns float32 [B][R][C][Z]."""
    c = context(device)
    h = as_batch(hp, np.float32)
    B, R, C, Z = h.shape
    sg, search, patch = _denoise_args(sigma, B, strength, search, patch)
    out = np.empty_like(h)
    c.check(c.L.vh_denoise(c.h, _ptr(h), R, C, Z, B, _ptr(sg), ct.c_float(strength), search, patch,
                           int(bool(rician)), _ptr(out)), "vh_denoise")
    return out


def _mask_u8(a):
    """Any dtype -> uint8 as it stands when it is uint8 already, else (a != 0) as 0 / 1."""
    a = np.asarray(a)
    return a if a.dtype == np.uint8 else (a != 0)


def edit_mask(mask, op, radius=1, device=0):
    """The per-slice disc morphology from host arrays (vh_edit_mask; the spec is in
    include/vent_hip.h): ``mask`` a 3-D volume or a 4-D batch of any dtype, nonzero counting as set;
    ``op`` 'erode' | 'dilate' | 'open' | 'close'; ``radius`` 0..5, a scalar or one int per study (a
    study of radius 0 comes back as it went in).  Returns uint8 [B][R][C][Z]."""
    c = context(device)
    m = as_batch(_mask_u8(mask), np.uint8)
    B, R, C, Z = m.shape
    op, rad = _mask_edit_args(op, radius, B)
    out = np.empty_like(m)
    c.check(c.L.vh_edit_mask(c.h, _ptr(m), R, C, Z, B, op, _ptr(rad), _ptr(out), None), "vh_edit_mask")
    return out


def segment(proton, thresh=None, open_radius=1, device=0, count=False):
    """The lungs from proton images on the host (vh_segment; the spec is in include/vent_hip.h):
    ``proton`` a 3-D volume or a 4-D batch; ``thresh`` None (the Otsu threshold of every study), a
    scalar or one value per study; ``open_radius`` 0..5, a scalar or one int per study.  Returns
    (mask uint8 [B][R][C][Z], the thresholds used float32 [B]), and with ``count`` the voxel counts
    int64 [B] as a third.  IndexError when Otsu is asked for a study that has no threshold."""
    c = context(device)
    x = as_batch(proton, np.float32)
    B, R, C, Z = x.shape
    th, rad = _segment_args(thresh, open_radius, B, (R, C, Z))
    out = np.empty(x.shape, np.uint8)
    used = np.zeros(B, np.float32)
    cnt = np.zeros(B, np.int64) if count else None
    c.check(c.L.vh_segment(c.h, _ptr(x), R, C, Z, B, _ptr(th), _ptr(rad), _ptr(out), _ptr(used), _ptr(cnt)),
            "vh_segment")
    return (out, used, cnt) if count else (out, used)


def register(proton, hp, search=(4, 4, 1), apply=False, device=0):
    """The proton registered to the xenon image from host arrays (vh_register; the spec is in
    include/vent_hip.h): ``proton`` and ``hp`` 3-D volumes or 4-D batches of one shape.  Returns (best int32
    [B][3], score float64 [B][2Sz+1][2Sr+1][2Sc+1], status int32 [B]), and with ``apply`` the proton
    shifted by best, float32 [B][R][C][Z], as a fourth."""
    p = as_batch(proton, np.float32)
    x = as_batch(hp, np.float32)
    if p.shape != x.shape:
        raise ValueError(f"register: proton {p.shape} and hp {x.shape} differ in shape")
    B, R, C, Z = p.shape
    se = _register_args(search, (R, C, Z))   # (before any device call)
    c = context(device)
    score = np.zeros((B,) + _score_shape(se), np.float64)
    best = np.zeros((B, 3), np.int32)
    status = np.zeros(B, np.int32)
    out = np.empty(p.shape, np.float32) if apply else None
    c.check(c.L.vh_register(c.h, _ptr(p), _ptr(x), R, C, Z, B, _ptr(se), _ptr(score), _ptr(best), _ptr(status),
                            _ptr(out)), "vh_register")
    return (best, score, status, out) if apply else (best, score, status)


def resample(src, dst_shape, maps, device=0):
    """Volumes resampled from their own grid onto another from host arrays (vh_resample; the spec is in
    include/vent_hip.h): ``src`` a 3-D volume or a 4-D batch of one shape, ``dst_shape`` (R, C, Z),
    ``maps`` one [3][2] map of (scale, offset) per axis (grid_map makes one) or one per study.  Returns
    float32 [B][R][C][Z]."""
    x = as_batch(src, np.float32)
    B = x.shape[0]
    R, C, Z = _shape3(dst_shape, "resample: dst_shape")
    if R < 2 or C < 2:
        raise ValueError(f"resample: dst_shape needs R >= 2 and C >= 2, got {dst_shape!r}")
    m = _resample_args(maps, B, x.shape[1:])   # (before any device call)
    c = context(device)
    shape = np.asarray(x.shape[1:], np.int64)
    out = np.empty((B, R, C, Z), np.float32)
    c.check(c.L.vh_resample(c.h, _ptr(x), _ptr(shape), R, C, Z, B, _ptr(m), _ptr(out)), "vh_resample")
    return out


def register_maps(src, hp, lists, home=None, device=0):
    """The fine registration from host arrays (vh_register_maps; the spec is in include/vent_hip.h): ``src``
    the protons on their own grid, a 3-D volume or a 4-D batch of one shape, ``hp`` the xenon volumes,
    ``lists`` the r, c and z candidate lists of (scale, offset) (map_candidates makes them).  Returns (best
    int32 [B][3], best_map float64 [B][3][2], score float64 [B][Kz][Kr][Kc], status int32 [B])."""
    s = as_batch(src, np.float32)
    x = as_batch(hp, np.float32)
    if s.shape[0] != x.shape[0]:
        raise ValueError(f"register_maps: {s.shape[0]} sources and {x.shape[0]} xenon volumes")
    B, R, C, Z = x.shape
    shape = np.asarray(_shape3(s.shape[1:], "register_maps: the source shape", RESAMPLE_MAX_SRC), np.int64)
    count, am, h = _register_maps_args(lists, B, home)   # (before any device call)
    c = context(device)
    score = np.zeros((B, int(count[2]), int(count[0]), int(count[1])), np.float64)
    best = np.zeros((B, 3), np.int32)
    best_map = np.zeros((B, 3, 2), np.float64)
    status = np.zeros(B, np.int32)
    c.check(c.L.vh_register_maps(c.h, _ptr(s), _ptr(shape), _ptr(x), R, C, Z, B, _ptr(count), _ptr(am), _ptr(h),
                                 _ptr(score), _ptr(best), _ptr(best_map), _ptr(status)), "vh_register_maps")
    return best, best_map, score, status


def ci(defect, table, minvox, device=0, shell=True, out=None):
    """table: vent_analysis_amd.sphere.SphereTable for this shape (kept in HBM per context after
    the first call).  Returns (ci f64, scalar[B], shell int32 or None).  The map goes into a pooled
    page-locked buffer the scatter kernel writes directly (vh_host_alloc), or into ``out`` (a
    C-contiguous f64 array of the batch's shape: then through a device map and one copy)."""
    c = context(device)
    d = np.asarray(defect)
    if d.dtype == np.bool_:
        d = d.view(np.uint8)   # (no copy: the kernels test != 0)
    elif d.dtype != np.uint8:
        d = d != 0
    d = as_batch(d, np.uint8)   # a u8 map goes in as it is (nonzero = defect, CI.py:37)
    B, R, C, Z = d.shape
    if out is None:
        out = c.pinned.array((B, R, C, Z), np.float64)   # page-locked, device-mapped: no copy
    elif out.dtype != np.float64 or out.size != B * R * C * Z or not out.flags.c_contiguous:
        raise ValueError("ci: out must be a C-contiguous float64 array of the batch's size")
    sh = np.empty((B, R, C, Z), np.int32) if shell else None
    sc = np.zeros(B, np.float64)
    with c.ci_lock:
        th = c.ci_table(table, R, C)
        c.check(c.L.vh_ci_tab(c.h, _ptr(d), R, C, Z, B, th, ct.c_double(minvox), _ptr(out), _ptr(sc),
                              _ptr(sh)), "vh_ci_tab")
    return out, sc, sh


def ci_expand(shell, radii, minvox):
    """The float64 CI map of a shell map (Batch.download_ci(maps="shell")): radii[shell] * minvox on
    the defect voxels (shell >= 0), 0.0 elsewhere -- the product CI.py:105 forms, so it equals the
    device's float64 map bit for bit at a quarter of the transfer."""
    sh = np.asarray(shell)
    if not np.issubdtype(sh.dtype, np.integer):
        raise ValueError(f"ci_expand: shell must be an integer array, got {sh.dtype}")
    r = np.asarray(radii, dtype=np.float64)
    if sh.size and int(sh.max()) >= r.shape[0]:
        raise ValueError(f"ci_expand: shell {int(sh.max())} is past the table's {r.shape[0]} radii")
    on = sh >= 0
    return np.where(on, r[np.where(on, sh, 0)] * float(minvox), 0.0)


def ctx_profile(on, device=0):
    """Time the kernel classes of the host-buffer entry points (vh_ci, ...) on this device's
    context (vh_ctx_profile); switching discards earlier timings."""
    c = context(device)
    c.check(c.L.vh_ctx_profile(c.h, 1 if on else 0), "vh_ctx_profile")


def ctx_kernel_time(name, device=0):
    """(total ms, launches) of a kernel class timed since ctx_profile(True)."""
    c = context(device)
    ms, n = ct.c_double(), ct.c_int64()
    c.check(c.L.vh_ctx_kernel_time(c.h, name.encode(), ct.byref(ms), ct.byref(n)), "vh_ctx_kernel_time")
    return ms.value, n.value


def overlay(n4, defect, device=0):
    """exportDICOM pixel data (vh_overlay): uint8 [B][Z][R][C][3] for (B, R, C, Z) inputs (a
    single volume gives [Z][R][C][3])."""
    c = context(device)
    single = np.ndim(n4) == 3
    n = as_batch(n4, np.float32)
    d = as_batch(defect, np.uint8) if np.asarray(defect).dtype == np.uint8 else \
        as_batch(np.where(np.asarray(defect) == 1, 1, np.where(np.asarray(defect) == 0, 0, 2)), np.uint8)
    B, R, C, Z = n.shape
    out = np.empty((B, Z, R, C, 3), np.uint8)
    c.check(c.L.vh_overlay(c.h, _ptr(n), _ptr(d), R, C, Z, B, _ptr(out)), "vh_overlay")
    return out[0] if single else out


def montage(proton, hp, n4, mask_border, defect, ci, parula, crop, device=0):
    """screenShot's montage array (vh_montage): uint8 [7 nr][ns nc][3].  crop = (r0, nr, c0, nc,
    s0, ns); ci None = the blank CI panel."""
    c = context(device)

    def fl(a):
        a = np.asarray(a)
        if a.dtype == np.float64:
            return np.ascontiguousarray(a), 1
        return np.ascontiguousarray(a, dtype=np.float32), 0
    p, p64 = fl(proton)
    h, h64 = fl(hp)
    n = np.ascontiguousarray(n4, dtype=np.float32)
    R, C, Z = n.shape
    mb = np.ascontiguousarray(np.asarray(mask_border) != 0, dtype=np.uint8)
    df = np.ascontiguousarray(np.asarray(defect) != 0, dtype=np.uint8)
    ci64 = None if ci is None else np.ascontiguousarray(ci, dtype=np.float64)
    pal = np.ascontiguousarray(parula, dtype=np.float64)
    cr = np.ascontiguousarray(crop, dtype=np.int64)
    img = np.empty((7 * int(cr[1]), int(cr[5]) * int(cr[3]), 3), np.uint8)
    c.check(c.L.vh_montage(c.h, R, C, Z, _ptr(p), p64, _ptr(h), h64, _ptr(n), _ptr(mb), _ptr(df),
                           _ptr(ci64), _ptr(pal), pal.shape[0], _ptr(cr), _ptr(img)), "vh_montage")
    return img


def montage_views(buf, crop, offset, status):
    """Batch.montage's images out of the compact buffer: study i's uint8 [7 nr][ns nc][3] is the
    21 nr nc ns bytes at offset[i] (crop[i] = r0, nr, c0, nc, s0, ns); None where status[i] != VH_OK.
    Views of ``buf``, no copies."""
    out = []
    for (r0, nr, c0, nc, s0, ns), o, st in zip(np.asarray(crop).tolist(), np.asarray(offset).tolist(),
                                               np.asarray(status).tolist()):
        if st != VH_OK:
            out.append(None)
            continue
        n = 21 * nr * nc * ns
        if o + n > buf.shape[0]:
            raise ValueError(f"montage_views: an image of {n} bytes at {o} is past the buffer's {buf.shape[0]}")
        out.append(buf[o:o + n].reshape(7 * nr, ns * nc, 3))
    return out


def recon(raw_k, device=0):
    """process_RAW's image (vh_recon, Vent_Analysis.py:537-540): complex k-space [n0][n1][nz] ->
    complex128 [n1][n0][nz] = transpose(fftshift(fft2(fftshift(slice))), (1, 0, 2))[:, ::-1, :].
    The transform runs in complex128 whatever the input precision (numpy 1.23, the reference pin,
    computes every FFT in double)."""
    c = context(device)
    k = np.asarray(raw_k)
    if k.ndim != 3:
        raise ValueError(f"raw k-space must be 3-D (cols, lines, slices), got shape {k.shape}")
    k = np.ascontiguousarray(k, dtype=np.complex128)
    n0, n1, nz = k.shape
    out = np.empty((n1, n0, nz), np.complex128)
    c.check(c.L.vh_recon(c.h, _ptr(k), n0, n1, nz, _ptr(out)), "vh_recon")
    return out


class Batch:
    """Device-resident batch of studies (vh_batch): upload once, run the whole pipeline on the
    GPU, download results.  Used by bench.py and for cohort processing."""

    def __init__(self, R, C, Z, n, device=0):
        self.ctx = context(device)
        self.L = self.ctx.L
        self.shape = (int(n), int(R), int(C), int(Z))
        h = _P()
        self.ctx.check(self.L.vh_batch_create(self.ctx.h, R, C, Z, n, ct.byref(h)),
                       "vh_batch_create")
        self.h = h
        _live.add(self)

    def close(self):
        if getattr(self, "h", None):
            self.L.vh_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, hp, mask):
        """``hp`` None uploads the masks alone (the resident HPvent stays as it is)."""
        h = None if hp is None else np.ascontiguousarray(hp, dtype=np.float32)
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        if (h is not None and h.shape != self.shape) or m.shape != self.shape:
            raise ValueError(f"batch expects {self.shape}")
        self.ctx.check(self.L.vh_batch_upload(self.h, _ptr(h), _ptr(m)), "vh_batch_upload")

    @staticmethod
    def options(do_n4=True, thresh=0.6, do_snr=True, do_kmeans=True, do_cohort=False,
                profile=False, vox=(1.0, 1.0, 1.0), n4_subbatch=0, morph3d=False,
                n4_mode=0, **n4kw) -> RunOpts:
        o = RunOpts()
        lib().vh_default_run_opts(ct.byref(o))
        o.do_n4 = int(bool(do_n4))
        o.n4 = n4_params(**n4kw)
        o.thresh = thresh
        o.do_snr = int(bool(do_snr))
        o.do_kmeans = int(bool(do_kmeans))
        o.do_cohort = int(bool(do_cohort))
        o.profile = int(bool(profile))
        for i in range(3):
            o.vox[i] = float(vox[i])
        o.n4_subbatch = int(n4_subbatch)
        o.morph3d = int(bool(morph3d))
        o.n4_mode = {"auto": 0, "sweep": 1, "study": 2, "grid": 3}.get(n4_mode, n4_mode)
        return o

    def run(self, opts: RunOpts):
        self.ctx.check(self.L.vh_batch_run(self.h, ct.byref(opts)), "vh_batch_run")

    def sync(self):
        self.ctx.check(self.L.vh_batch_sync(self.h), "vh_batch_sync")

    def download(self, n4=False, maps=True):
        B = self.shape[0]
        out_n4 = np.empty(self.shape, np.float32) if n4 else None
        d = np.empty(self.shape, np.uint8) if maps else None
        bo = np.empty(self.shape, np.uint8) if maps else None
        lb = np.empty(self.shape, np.uint8) if maps else None
        res = (VdpResult * B)()
        self.ctx.check(self.L.vh_batch_download(self.h, _ptr(out_n4), _ptr(d), _ptr(bo), _ptr(lb),
                                                ct.cast(res, ct.c_void_p)), "vh_batch_download")
        return out_n4, d, bo, lb, list(res)

    def upload_defect(self, d):
        """Replace the resident defect maps (nonzero = defect): the CI of edited or stored maps."""
        d = np.asarray(d)
        if d.dtype != np.uint8:
            d = d != 0
        d = np.ascontiguousarray(d, dtype=np.uint8)
        if d.shape != self.shape:
            raise ValueError(f"batch expects {self.shape}")
        self.ctx.check(self.L.vh_batch_set_defect(self.h, _ptr(d)), "vh_batch_set_defect")

    def select_defect(self, source, medfilt=1):
        """Rebuild the resident defect map and border from the last run's N4 and scalars (enqueue
        only): ``source`` 'mean' | 'lb' | 'kmeans' (or VH_DEFECT_*), ``medfilt`` 0 raw, 1 the per-slice
        3x3 median, 2 the 3x3x3 majority with the 3-D border.  ci(), download() and download_defect()
        then see the selected map; the run's results stay as they are."""
        self.ctx.check(self.L.vh_batch_select_defect(self.h, defect_source(source), int(medfilt)),
                       "vh_batch_select_defect")

    def download_defect(self, km=False):
        """(defect, border, count) of the resident maps -- uint8 [B][R][C][Z] twice and int64 [B] --
        plus the k-means label map (0 off-mask, else 1 + cluster) when ``km``."""
        d = np.empty(self.shape, np.uint8)
        bo = np.empty(self.shape, np.uint8)
        lab = np.empty(self.shape, np.uint8) if km else None
        cnt = np.zeros(self.shape[0], np.int64)
        self.ctx.check(self.L.vh_batch_download_defect(self.h, _ptr(d), _ptr(bo), _ptr(lab), _ptr(cnt)),
                       "vh_batch_download_defect")
        return (d, bo, cnt, lab) if km else (d, bo, cnt)

    def km_cuts(self):
        """float32 [B][3]: the smallest value of k-means clusters 1..3 of each study, +inf where
        the cut is at n (the cluster and all above it are empty)."""
        cuts = np.zeros((self.shape[0], 3), np.float32)
        self.ctx.check(self.L.vh_batch_km_cuts(self.h, _ptr(cuts)), "vh_batch_km_cuts")
        return cuts

    def ci(self, vox, Rmax=50, table=None):
        """Enqueue the cluster index of the resident defect maps (the last run's, or
        upload_defect's) on the batch's stream; download_ci fetches it.  ``table``: a
        sphere.SphereTable for this shape (default: compact_table_for(vox, Rmax, shape))."""
        from .sphere import compact_table_for
        _, R, C, Z = self.shape
        if table is None:
            table = compact_table_for(vox, Rmax, (R, C, Z))
        minvox = float(np.min(vox))
        with self.ctx.ci_lock:   # the handle is not evicted between the lookup and the enqueue
            th = self.ctx.ci_table(table, R, C)
            self.ctx.check(self.L.vh_batch_ci(self.h, th, ct.c_double(minvox)), "vh_batch_ci")
        self.ci_radii = table.radii
        self.ci_minvox = minvox

    def download_ci(self, maps="shell"):
        """(map, scalars, status) of the last ci(): the int16 shell map (``maps="shell"``: -1
        off-defect, else the index into ``ci_radii``; ci_expand gives the float64 map), the float64
        CI map (``"f64"``) or None; scalars float64 [B], NaN where status != 0; status int32 [B]:
        VH_OK, VH_ERR_EMPTY (no defect voxels) or VH_ERR_MAXRADIUS per study."""
        if maps not in ("shell", "f64", None):
            raise ValueError('download_ci: maps is "shell", "f64" or None')
        B = self.shape[0]
        f64 = np.empty(self.shape, np.float64) if maps == "f64" else None
        sh = np.empty(self.shape, np.int16) if maps == "shell" else None
        sc = np.zeros(B, np.float64)
        status = np.zeros(B, np.int32)
        self.ctx.check(self.L.vh_batch_download_ci(self.h, _ptr(f64), _ptr(sh), _ptr(sc), _ptr(status)),
                       "vh_batch_download_ci")
        sc[status != VH_OK] = np.nan
        return (f64 if maps == "f64" else sh), sc, status

    def overlay(self):
        """exportDICOM's pixel data of every study (vh_batch_overlay): uint8 [B][Z][R][C][3], rendered
        on the device from the N4 the last run's chain read and the resident defect maps (the run's,
        upload_defect's or select_defect's) -- study i's block equals _lib.overlay of its downloaded
        N4 and defect map.  Needs a run (ValueError otherwise)."""
        B, R, C, Z = self.shape
        self.ctx.check(self.L.vh_batch_overlay(self.h), "vh_batch_overlay")
        out = self.ctx.pinned.array((B, Z, R, C, 3), np.uint8)   # page-locked: the D2H runs at the link rate
        self.ctx.check(self.L.vh_batch_download_overlay(self.h, _ptr(out)), "vh_batch_download_overlay")
        return out

    def montage_layout(self):
        """(crop int64 [B][6], offset int64 [B + 1], status int32 [B]) of the batch's montages
        (vh_batch_montage_layout): crop[i] = (r0, nr, c0, nc, s0, ns) is cropToData(mask, border=5) of
        study i, offset[i] the byte at which its image starts in the compact buffer, offset[B] the
        buffer's size; status[i] is VH_ERR_EMPTY (zeros, no image) where the reference would raise
        IndexError.  Needs a run."""
        B = self.shape[0]
        crop = np.zeros((B, 6), np.int64)
        off = np.zeros(B + 1, np.int64)
        status = np.zeros(B, np.int32)
        self.ctx.check(self.L.vh_batch_montage_layout(self.h, _ptr(crop), _ptr(off), _ptr(status)),
                       "vh_batch_montage_layout")
        return crop, off, status

    def montage(self, parula, proton=None):
        """screenShot's montage array of every study, rendered on the device from the resident
        HPvent, N4, mask and defect maps (vh_batch_montage): (images, status).  images[i] is uint8
        [7 nr][ns nc][3] over study i's crop (a view of one compact buffer) or None where status[i] !=
        VH_OK: VH_ERR_EMPTY (no crop) or VH_ERR_INDEX (a CI colour index past ``parula``).  The CI panel
        is drawn when ci() was enqueued after the last run / upload_defect / select_defect, else it is
        the blank CI panel.  ``proton`` [B][R][C][Z] (None: zeros) is converted to float32, so a
        float64 proton is normalised in float32 here, unlike Vent_Analysis.screenShot, which
        normalises a float64 proton in float64."""
        pal = np.ascontiguousarray(parula, dtype=np.float64)
        if pal.ndim != 2 or pal.shape[1] != 3:
            raise ValueError(f"montage: parula must be [rows][3], got shape {pal.shape}")
        p = None
        if proton is not None:
            p = np.ascontiguousarray(proton, dtype=np.float32)
            if p.shape != self.shape:
                raise ValueError(f"batch expects {self.shape}")
        crop, off, lstatus = self.montage_layout()
        self.ctx.check(self.L.vh_batch_montage(self.h, _ptr(p), _ptr(pal), pal.shape[0]), "vh_batch_montage")
        buf = self.ctx.pinned.array((int(off[-1]),), np.uint8) if off[-1] else np.empty(0, np.uint8)
        status = np.zeros(self.shape[0], np.int32)
        self.ctx.check(self.L.vh_batch_download_montage(self.h, _ptr(buf), _ptr(status)),
                       "vh_batch_download_montage")
        return montage_views(buf, crop, off, status), status

    def distribution(self, norm="p99", bins=1024, hi=1.5):
        """Enqueue the ventilation distribution of every study (vh_batch_distribution): the histogram
        of float32(N4 / d) over mask != 0 in ``bins`` bins of [0, hi) -- d the run's mean anchor
        (``norm`` 'mean') or 99th percentile ('p99') -- and the per-slice counts of mask, defect and LB
        class voxels, from the buffers the last run left resident and the defect map as it stands.
        Read-only; download_distribution fetches the last call's result.  Needs a run."""
        self.ctx.check(self.L.vh_batch_distribution(self.h, norm_source(norm), int(bins), ct.c_float(hi)),
                       "vh_batch_distribution")
        self._dist = (int(bins), float(hi))

    def download_distribution(self):
        """The last distribution() as a dict: ``hist`` uint32 [B][bins]; ``outside`` int64 [B][2], the
        masked voxels below 0 and those at or above hi (NaN included); ``slice_counts`` int64
        [B][Z][8] with columns mask, defect, LB class 1..6; ``edges`` float64 [bins + 1], for display."""
        bins, hi = getattr(self, "_dist", (0, 1.0))
        B, _, _, Z = self.shape
        hist = np.zeros((B, bins), np.uint32)
        outside = np.zeros((B, 2), np.int64)
        sl = np.zeros((B, Z, VH_DIST_COLS), np.int64)
        self.ctx.check(self.L.vh_batch_download_distribution(self.h, _ptr(hist), _ptr(outside), _ptr(sl)),
                       "vh_batch_download_distribution")
        return dict(hist=hist, outside=outside, slice_counts=sl, edges=dist_edges(bins, hi))

    def heterogeneity(self, radius=1, min_count=None, bins=100, hi=1.0, exclude_defect=False):
        """Enqueue the local ventilation heterogeneity of every study (vh_batch_heterogeneity; the
        spec is in include/vent_hip.h): the coefficient of variation of the volume the last run's chain
        read over the masked pixels of the (2 radius + 1)^2 in-plane window, where at least
        ``min_count`` (None: a majority of the window) of them are set, and its histogram in ``bins``
        bins of [0, hi).  ``exclude_defect`` takes the resident defect map's voxels out of the mask.
        Read-only; download_heterogeneity fetches the last call's result.  Needs a run."""
        radius, min_count, bins, hi = _heterogeneity_args(radius, min_count, bins, hi)
        self.ctx.check(self.L.vh_batch_heterogeneity(self.h, radius, min_count, bins, ct.c_float(hi),
                                                     int(bool(exclude_defect))), "vh_batch_heterogeneity")
        self._het = (bins, hi)

    def download_heterogeneity(self, map=True):
        """The last heterogeneity() as a dict: ``map`` float32 [B][R][C][Z] (+0 off the mask, -1 where
        the mask is set but there is no value, else the CoV; None with ``map=False``: only counts come
        back); ``hist`` uint32 [B][bins]; ``edges`` float64 [bins + 1], for display; ``stats`` int64
        [B][4]: n_in, n_over (at or above hi, NaN included), n_none, sum_fx; ``index`` float64 [B],
        het_index(stats)."""
        bins, hi = getattr(self, "_het", (0, 1.0))
        B = self.shape[0]
        out = np.empty(self.shape, np.float32) if map else None
        hist = np.zeros((B, bins), np.uint32)
        stats = np.zeros((B, 4), np.int64)
        self.ctx.check(self.L.vh_batch_download_heterogeneity(self.h, _ptr(out), _ptr(hist), _ptr(stats)),
                       "vh_batch_download_heterogeneity")
        return dict(map=out, hist=hist, edges=dist_edges(bins, hi) if bins else None, stats=stats,
                    index=het_index(stats))

    def core_rind(self, edges=(1.5, 3.5), with_defect=True, thresholds=None):
        """Enqueue the core-rind analysis of every study (vh_batch_core_rind; the spec is in
        include/vent_hip.h): the exact squared in-plane distance D2 of every mask voxel to the mask's
        edge (the slice border is an edge), and the mask and defect voxels of the depth bands that
        ``edges`` (pixels, increasing; depth_thresholds) or ``thresholds`` (D2 values as they are)
        separate, band 0 the outermost rind.  ``with_defect`` counts the resident defect map as it
        stands (needs a run or upload_defect); without it the defect column is 0.  Read-only;
        download_core_rind fetches the last call's result."""
        thr = _core_rind_args(edges, thresholds)
        self.ctx.check(self.L.vh_batch_core_rind(self.h, _ptr(thr), thr.size, int(bool(with_defect))),
                       "vh_batch_core_rind")
        self._cr = thr

    def download_core_rind(self, map=True):
        """The last core_rind() as a dict: ``d2`` uint16 [B][R][C][Z] = min(D2, 65535), 0 off the mask
        (None with ``map=False``: only counts come back); ``counts`` int64 [B][bands][2], the band's mask
        voxels and its defect voxels; ``stats`` int64 [B][2], n_mask and the largest D2 (unsaturated);
        ``thresholds`` uint16 [bands - 1]; ``band_vdp`` float64 [B][bands], 100 * defect / mask, NaN
        for an empty band."""
        thr = getattr(self, "_cr", np.zeros(0, np.uint16))
        B = self.shape[0]
        out = np.empty(self.shape, np.uint16) if map else None
        counts = np.zeros((B, thr.size + 1, 2), np.int64)
        stats = np.zeros((B, 2), np.int64)
        self.ctx.check(self.L.vh_batch_download_core_rind(self.h, _ptr(out), _ptr(counts), _ptr(stats)),
                       "vh_batch_download_core_rind")
        return dict(d2=out, counts=counts, stats=stats, thresholds=thr.copy(), band_vdp=band_vdp(counts))

    def components(self, source="defect", conn=6, edges=()):
        """Enqueue the connected components of every study (vh_batch_components; the spec is in
        include/vent_hip.h): of the resident defect map as it stands (``source`` 'defect': needs a run
        or upload_defect) or of the resident mask ('mask'), under ``conn`` 4 | 8 (every slice on its
        own) | 6 | 26 neighbours.  ``edges`` (ints, increasing, >= 2) separate the size classes of the
        counts.  Read-only; download_components fetches the last call's result."""
        source, conn, e = _components_args(source, conn, edges)
        self.ctx.check(self.L.vh_batch_components(self.h, source, conn, _ptr(e), e.size), "vh_batch_components")
        self._cc = e

    def download_components(self, root=True, size=True):
        """The last components() as a dict: ``root`` int32 [B][R][C][Z], the smallest linear index of
        the voxel's component, -1 off the set; ``size`` uint32 [B][R][C][Z], the component's voxels, 0
        off the set (each None when not asked for: only the summary comes back); ``counts`` int64
        [B][classes][2], the components of each size class and their voxels; ``stats`` int64 [B][4] =
        n_set, n_comp, the largest component's size (0: none) and root (-1: none); ``edges`` uint32."""
        e = getattr(self, "_cc", np.zeros(0, np.uint32))
        B = self.shape[0]
        r = np.empty(self.shape, np.int32) if root else None
        sz = np.empty(self.shape, np.uint32) if size else None
        counts = np.zeros((B, e.size + 1, 2), np.int64)
        stats = np.zeros((B, 4), np.int64)
        self.ctx.check(self.L.vh_batch_download_components(self.h, _ptr(r), _ptr(sz), _ptr(counts), _ptr(stats)),
                       "vh_batch_download_components")
        return dict(root=r, size=sz, counts=counts, stats=stats, edges=e.copy())

    def defect_table(self, min_size=1, max_rows=64, norm=None):
        """Enqueue the defect table of every study (vh_batch_defect_table; the spec is in
        include/vent_hip.h): one row per component of the last components() with at least ``min_size``
        voxels (a scalar or one int per study), largest first, at most ``max_rows`` (1..1024).  ``norm``
        'mean' | 'p99' fills the signal columns from the run's N4 (needs a run); None leaves them 0.
        Read-only; download_defect_table fetches the last call's result."""
        ms, max_rows, norm = _defect_table_args(min_size, max_rows, norm, self.shape[0])
        self.ctx.check(self.L.vh_batch_defect_table(self.h, _ptr(ms), max_rows, norm), "vh_batch_defect_table")
        self._dt = max_rows

    def download_defect_table(self):
        """The last defect_table() as a dict: ``rows`` int64 [B][max_rows][18] with the columns of
        DT_COLUMNS (an unused row: -1, then zeros); ``stats`` int64 [B][4] = n_rows, n_qualifying, the
        voxels in the rows, the voxels in the qualifying components; ``truncated`` bool [B], n_rows <
        n_qualifying.  table_metrics() turns rows into mL, mm and signal means."""
        B, n = self.shape[0], getattr(self, "_dt", 1)
        rows = np.zeros((B, n, VH_DT_COLS), np.int64)
        stats = np.zeros((B, 4), np.int64)
        self.ctx.check(self.L.vh_batch_download_defect_table(self.h, _ptr(rows), _ptr(stats)),
                       "vh_batch_download_defect_table")
        return dict(rows=rows, stats=stats, truncated=stats[:, 0] < stats[:, 1])

    def zones(self, parts=(3, 1, 1), lateral=True, by="extent", labels=None, n_zones=None, norm="mean", bins=100,
              hi=1.5):
        """Enqueue the regional analysis of every study (vh_batch_zones; the spec is in
        include/vent_hip.h): a zone map and per zone the mask, defect and LB class counts and the
        histogram of float32(N4 / d) in ``bins`` bins of [0, hi).  Geometric zones: ``parts`` (rows,
        columns, slices) cut the mask's bounding box ``by`` 'extent' or by voxel 'count', and
        ``lateral`` splits the columns into the left and the right lung at the emptiest column of the
        middle half (``parts[1]`` must then be 1).  ``labels``, uint8 [B][R][C][Z], gives the caller's
        zones 1..``n_zones`` instead (None: the largest label); any other byte on the mask is zone 0.
        Read-only; download_zones fetches the last call's result.  Needs a run."""
        a = _zones_args(parts, lateral, by, labels, n_zones, norm, bins, hi, self.shape)
        self.ctx.check(self.L.vh_batch_zones(self.h, _ptr(a["labels"]), a["n_zones"], _ptr(a["parts"]), a["lateral"],
                                             a["by"], a["norm"], a["bins"], ct.c_float(a["hi"])), "vh_batch_zones")
        a["labels"] = None
        self._zn = a

    def download_zones(self, map=True):
        """The last zones() as a dict: ``map`` uint8 [B][R][C][Z], the zone 1..K of every mask voxel (0
        off the mask, and for a mask voxel no label claims; None with ``map=False``: only counts come
        back); ``counts`` int64 [B][K + 1][8] with columns mask, defect, LB class 1..6; ``hist`` uint32
        [B][K + 1][bins]; ``edges`` float64 [bins + 1], for display; ``stats`` int64 [B][K + 1][4]: n_in,
        n_below, n_over, sum_fx; ``geom`` int32 [B][8]: lo_r, hi_r, lo_c, hi_c, lo_z, hi_z, the split
        column (-1: none), 0; ``zone_vdp`` float64 [B][K + 1], 100 * defect / mask, NaN for an empty
        zone; ``zone_mean`` float64 [B][K + 1], the mean normalised signal; ``n_zones`` K."""
        a = getattr(self, "_zn", dict(K=0, bins=0, hi=1.0))
        B, K1 = self.shape[0], a["K"] + 1
        out = self.ctx.pinned.array(self.shape, np.uint8) if map else None   # page-locked: the link rate
        counts = np.zeros((B, K1, VH_ZONE_COLS), np.int64)
        hist = np.zeros((B, K1, a["bins"]), np.uint32)
        stats = np.zeros((B, K1, 4), np.int64)
        geom = np.zeros((B, 8), np.int32)
        self.ctx.check(self.L.vh_batch_download_zones(self.h, _ptr(out), _ptr(counts), _ptr(hist), _ptr(stats),
                                                      _ptr(geom)), "vh_batch_download_zones")
        if not a["bins"]:   # (unreachable: the library refuses a download before any zones())
            raise ValueError("download_zones: zones() has not been called")
        return _zones_dict(a, out, counts, hist, stats, geom)

    def filter_components(self, source="defect", conn=6, min_size=1, keep_largest=0):
        """Clear the small components of the resident defect map or mask (vh_batch_filter_components):
        a component stays when it has ``min_size`` voxels and, with ``keep_largest`` = k in 1..8, is among
        the k largest of its study (ties: the smaller root first); each a scalar or one int per study.
        'mask' puts the batch back where upload() left it, like edit_mask; 'defect' rebuilds the
        resident border and leaves the batch as upload_defect does (download_defect's count stays the
        run's).  A components() result is discarded.  Returns ``kept`` int64 [B][2] = components kept,
        voxels kept; waits."""
        B = self.shape[0]
        source, conn, ms, kl = _filter_components_args(source, conn, min_size, keep_largest, B)
        kept = np.zeros((B, 2), np.int64)
        self.ctx.check(self.L.vh_batch_filter_components(self.h, source, conn, _ptr(ms), _ptr(kl), _ptr(kept)),
                       "vh_batch_filter_components")
        return kept

    def noise_sigma(self):
        """float32 [B]: the noise of each resident HPvent (vh_batch_noise_sigma), sqrt(S2 / (2 N))
        over the voxels calculate_SNR counts as noise; NaN where the SNR is undefined.  Call it after
        upload (after a run it discards the run's results, like denoise)."""
        out = np.zeros(self.shape[0], np.float32)
        self.ctx.check(self.L.vh_batch_noise_sigma(self.h, _ptr(out)), "vh_batch_noise_sigma")
        return out

    def denoise(self, sigma=None, strength=2.0, search=3, patch=1, rician=False):
        """Enqueue the in-plane non-local-means filter (vh_batch_denoise; the spec is in
        include/vent_hip.h): the resident HPvent becomes its denoised volume, which the next run()
        reads.  ``sigma`` is a scalar or one value per study; None estimates it with noise_sigma()
        first and raises ValueError if the estimate is NaN for any study.  Returns the sigma used,
        float32 [B].  After a run, the calls that need a run raise ValueError until the next one."""
        if sigma is None:
            sigma = self.noise_sigma()
            if np.isnan(sigma).any():
                raise ValueError(f"denoise: the noise estimate is undefined for studies "
                                 f"{np.flatnonzero(np.isnan(sigma)).tolist()}; pass sigma")
        sg, search, patch = _denoise_args(sigma, self.shape[0], strength, search, patch)
        self.ctx.check(self.L.vh_batch_denoise(self.h, _ptr(sg), ct.c_float(strength), search, patch,
                                               int(bool(rician))), "vh_batch_denoise")
        return sg

    def download_hp(self):
        """The resident HPvent as it stands (vh_batch_download_hp), float32 [B][R][C][Z]."""
        out = np.empty(self.shape, np.float32)
        self.ctx.check(self.L.vh_batch_download_hp(self.h, _ptr(out)), "vh_batch_download_hp")
        return out

    def edit_mask(self, op, radius=1):
        """Enqueue the per-slice disc morphology of the resident masks (vh_batch_edit_mask; the spec
        is in include/vent_hip.h): ``op`` 'erode' | 'dilate' | 'open' | 'close' (or VH_MASK_*),
        ``radius`` 0..5, a scalar or one int per study -- a study of radius 0 keeps its mask byte for
        byte, which is how one study is edited alone.  The next run() sees the edited masks.  After a
        run, the calls that need a run raise ValueError until the next one.  Returns the radii used,
        int32 [B]."""
        op, rad = _mask_edit_args(op, radius, self.shape[0])
        self.ctx.check(self.L.vh_batch_edit_mask(self.h, op, _ptr(rad)), "vh_batch_edit_mask")
        return rad

    def paint_mask(self, strokes, how="or"):
        """Paint on the resident masks (vh_batch_paint_mask): with p = (strokes != 0), [B][R][C][Z] of
        any dtype, the mask becomes s | p ('or'), s & ~p ('andnot'), s & p ('and') or s ^ p ('xor') as
        0 / 1 bytes.  Like edit_mask it puts the batch back where upload() left it."""
        how = paint_mode(how)
        p = np.ascontiguousarray(_mask_u8(strokes), dtype=np.uint8)
        if p.shape != self.shape:
            raise ValueError(f"batch expects {self.shape}")
        self.ctx.check(self.L.vh_batch_paint_mask(self.h, _ptr(p), how), "vh_batch_paint_mask")

    def download_mask(self, count=False):
        """The resident masks as they stand (vh_batch_download_mask), uint8 [B][R][C][Z]: after an
        upload, an edit or a run.  With ``count`` also the voxels != 0 of each study, int64 [B],
        counted on the device: (mask, count)."""
        out = self.ctx.pinned.array(self.shape, np.uint8)   # page-locked: the D2H runs at the link rate

        cnt = np.zeros(self.shape[0], np.int64) if count else None
        self.ctx.check(self.L.vh_batch_download_mask(self.h, _ptr(out), _ptr(cnt)), "vh_batch_download_mask")
        return (out, cnt) if count else out

    def upload_proton(self, proton):
        """The proton volumes of the batch, float32 [B][R][C][Z] (vh_batch_upload_proton): resident in
        a buffer of their own, as large as the HPvent's.  Invalidates nothing."""
        p = np.ascontiguousarray(proton, dtype=np.float32)
        if p.shape != self.shape:
            raise ValueError(f"batch expects {self.shape}")
        self.ctx.check(self.L.vh_batch_upload_proton(self.h, _ptr(p)), "vh_batch_upload_proton")

    def proton_threshold(self, stats=False):
        """float32 [B]: the Otsu threshold of each resident proton (vh_batch_proton_threshold; the spec
        is in include/vent_hip.h), NaN where it is undefined.  With ``stats`` also the maximum it scaled
        by and the 256-bin histogram it cut: (thresh, pmax float32 [B], hist uint32 [B][256])."""
        n = self.shape[0]
        th = np.zeros(n, np.float32)
        pmax = np.zeros(n, np.float32) if stats else None
        hist = np.zeros((n, 256), np.uint32) if stats else None
        self.ctx.check(self.L.vh_batch_proton_threshold(self.h, _ptr(th), _ptr(pmax), _ptr(hist)),
                       "vh_batch_proton_threshold")
        return (th, pmax, hist) if stats else th

    def segment(self, thresh=None, open_radius=1):
        """Enqueue the segmentation of the resident proton (vh_batch_segment; the spec is in
        include/vent_hip.h): the resident mask becomes, slice by slice, the pixels below ``thresh``
        that the slice border does not reach through such pixels, opened by the disc of
        ``open_radius`` (0..5, a scalar or one int per study; 0: no opening).  ``thresh`` is a scalar or
        one value per study; None takes proton_threshold() first and raises ValueError naming the
        studies whose threshold is NaN.  The next run() sees the new masks.  After a run, the calls that
        need a run raise ValueError until the next one.  Returns the thresholds used, float32 [B]."""
        _segment_args(1.0, open_radius, self.shape[0], self.shape[1:])   # (before any device call)
        if thresh is None:
            thresh = self.proton_threshold()
            if np.isnan(thresh).any():
                raise ValueError(f"segment: the Otsu threshold is undefined for studies "
                                 f"{np.flatnonzero(np.isnan(thresh)).tolist()}; pass thresh")
        th, rad = _segment_args(thresh, open_radius, self.shape[0], self.shape[1:])
        self.ctx.check(self.L.vh_batch_segment(self.h, _ptr(th), _ptr(rad)), "vh_batch_segment")
        return th

    def mask_overlap(self, other):
        """int64 [B][3]: per study the voxels != 0 of the resident mask, of ``other`` ([B][R][C][Z], any
        dtype) and of both, counted on the device (vh_batch_mask_overlap); Dice is 2 both / (a + b).
        Like paint_mask it puts the batch back where upload() left it."""
        o = np.ascontiguousarray(_mask_u8(other), dtype=np.uint8)
        if o.shape != self.shape:
            raise ValueError(f"batch expects {self.shape}")
        cnt = np.zeros((self.shape[0], 3), np.int64)
        self.ctx.check(self.L.vh_batch_mask_overlap(self.h, _ptr(o), _ptr(cnt)), "vh_batch_mask_overlap")
        return cnt

    def register(self, search=(4, 4, 1), hist=False):
        """Score every shift of the search window of the resident proton against the resident HPvent by
        mutual information (vh_batch_register; the spec is in include/vent_hip.h) and wait.  Returns
        (best int32 [B][3], score float64 [B][2Sz+1][2Sr+1][2Sc+1], status int32 [B]: 1 where a study has
        no voxel > 0 in one of the images, its scores NaN and its shift (0, 0, 0)); with ``hist`` also the
        joint histograms uint32 [B][2Sz+1][2Sr+1][2Sc+1][32][32].  Changes nothing another call reads."""
        se = _register_args(search, self.shape[1:])   # (before any device call)
        n = self.shape[0]
        score = np.zeros((n,) + _score_shape(se), np.float64)
        best = np.zeros((n, 3), np.int32)
        status = np.zeros(n, np.int32)
        self.ctx.check(self.L.vh_batch_register(self.h, _ptr(se), _ptr(score), _ptr(best), None, _ptr(status)),
                       "vh_batch_register")
        if not hist:
            return best, score, status
        h = np.zeros(score.shape + (REG_LEVELS, REG_LEVELS), np.uint32)
        self.ctx.check(self.L.vh_batch_download_register_hist(self.h, _ptr(h)), "vh_batch_download_register_hist")
        return best, score, status, h

    def shift_proton(self, shifts):
        """Enqueue a shift of the resident proton (vh_batch_shift): P'(v) = P(v + s) inside the volume, 0
        elsewhere, ``shifts`` one (dr, dc, dz) or one per study -- register()'s best puts the proton on the
        xenon's voxels.  Invalidates nothing.  Returns the shifts used, int32 [B][3]."""
        s = _shift_args(shifts, self.shape[0], self.shape[1:])
        self.ctx.check(self.L.vh_batch_shift(self.h, VH_SHIFT_PROTON, _ptr(s)), "vh_batch_shift")
        return s

    def shift_mask(self, shifts):
        """Enqueue the same shift of the resident masks (bytes move as they are).  The next run() sees
        the shifted masks; like edit_mask it puts the batch back where upload() left it."""
        s = _shift_args(shifts, self.shape[0], self.shape[1:])
        self.ctx.check(self.L.vh_batch_shift(self.h, VH_SHIFT_MASK, _ptr(s)), "vh_batch_shift")
        return s

    def download_proton(self):
        """The resident proton as it stands (vh_batch_download_proton), float32 [B][R][C][Z]."""
        out = np.empty(self.shape, np.float32)
        self.ctx.check(self.L.vh_batch_download_proton(self.h, _ptr(out)), "vh_batch_download_proton")
        return out

    def upload_proton_src(self, src):
        """The proton volumes on a grid of their own, float32 [B][Rs][Cs][Zs] with each dimension 1..1024
        (vh_batch_upload_proton_src): resident in a buffer of their own until the next such upload, so they
        can be resampled again with another map.  Invalidates nothing."""
        s = np.ascontiguousarray(src, dtype=np.float32)
        if s.ndim != 4 or s.shape[0] != self.shape[0]:
            raise ValueError(f"batch expects ({self.shape[0]}, Rs, Cs, Zs), got {s.shape}")
        shape = np.asarray(_shape3(s.shape[1:], "upload_proton_src: the source shape", RESAMPLE_MAX_SRC), np.int64)
        self.ctx.check(self.L.vh_batch_upload_proton_src(self.h, _ptr(s), _ptr(shape)), "vh_batch_upload_proton_src")
        self._src_shape = s.shape

    def resample_proton(self, maps):
        """Enqueue the resampling of the resident source onto the batch's grid (vh_batch_resample_proton; the
        spec is in include/vent_hip.h): the resident proton becomes the result, as after upload_proton().
        ``maps`` is one [3][2] map of (scale, offset) per axis (grid_map makes one) or one per study.
        Invalidates nothing else.  Returns the maps used, float64 [B][3][2]."""
        m = _resample_args(maps, self.shape[0])   # (before any device call)
        self.ctx.check(self.L.vh_batch_resample_proton(self.h, _ptr(m)), "vh_batch_resample_proton")
        return m

    def download_proton_src(self):
        """The resident source as it stands (vh_batch_download_proton_src), float32 [B][Rs][Cs][Zs]."""
        shape = getattr(self, "_src_shape", None)
        if shape is None:
            raise ValueError("download_proton_src: no proton source resident: upload_proton_src first")
        out = np.empty(shape, np.float32)
        self.ctx.check(self.L.vh_batch_download_proton_src(self.h, _ptr(out)), "vh_batch_download_proton_src")
        return out

    def register_maps(self, lists, home=None, hist=False):
        """Score a grid of candidate maps of the resident source proton against the resident HPvent by
        mutual information (vh_batch_register_maps; the spec is in include/vent_hip.h) and wait.  ``lists``
        is the r, the c and the z list of (scale, offset), each [K][2] for every study or [B][K][2]
        (map_candidates makes them); ``home`` the candidate ties fall to, the middle entries by default.
        Returns (best int32 [B][3] the picked (kr, kc, kz), best_map float64 [B][3][2] ready for
        resample_proton, score float64 [B][Kz][Kr][Kc], status int32 [B]: 1 where a study has no voxel > 0
        in one of the images, its scores NaN and its pick home); with ``hist`` also the joint histograms
        uint32 [B][Kz][Kr][Kc][32][32].  Changes nothing another call reads."""
        n = self.shape[0]
        count, am, h = _register_maps_args(lists, n, home)   # (before any device call)
        score = np.zeros((n, int(count[2]), int(count[0]), int(count[1])), np.float64)
        best = np.zeros((n, 3), np.int32)
        best_map = np.zeros((n, 3, 2), np.float64)
        status = np.zeros(n, np.int32)
        self.ctx.check(self.L.vh_batch_register_maps(self.h, _ptr(count), _ptr(am), _ptr(h), _ptr(score), _ptr(best),
                                                     _ptr(best_map), None, _ptr(status)), "vh_batch_register_maps")
        if not hist:
            return best, best_map, score, status
        hh = np.zeros(score.shape + (REG_LEVELS, REG_LEVELS), np.uint32)
        self.ctx.check(self.L.vh_batch_download_register_maps_hist(self.h, _ptr(hh)),
                       "vh_batch_download_register_maps_hist")
        return best, best_map, score, status, hh

    def cohort_hist(self):
        h = np.zeros(COHORT_BINS, np.uint64)
        self.ctx.check(self.L.vh_batch_cohort_hist(self.h, _ptr(h)), "vh_batch_cohort_hist")
        return h

    def cohort_allreduce(self):
        self.ctx.check(self.L.vh_batch_cohort_allreduce(self.h), "vh_batch_cohort_allreduce")

    def reset_timers(self):
        self.ctx.check(self.L.vh_batch_reset_timers(self.h), "vh_batch_reset_timers")

    def study_times(self):
        """Per-study wall time (us) of the last run's one-workgroup-per-study N4 kernel."""
        us = np.zeros(self.shape[0], np.float64)
        self.ctx.check(self.L.vh_batch_study_times(self.h, _ptr(us)), "vh_batch_study_times")
        return us

    def kernel_time(self, name):
        ms, n, by = ct.c_double(0), ct.c_int64(0), ct.c_double(0)
        self.ctx.check(self.L.vh_batch_kernel_time(self.h, name.encode(), ct.byref(ms),
                                                   ct.byref(n), ct.byref(by)),
                       "vh_batch_kernel_time")
        return ms.value, n.value, by.value


_batch_pool = {}   # (device, R, C, Z, n) -> idle Batch objects (pooled_batch)
_BATCH_POOL_KEEP = 2


class pooled_batch:
    """A device-resident batch of this shape for the length of a ``with`` block, reused across calls
    (the class's one-study calculate_VDP: creating a batch allocates its device workspace, which cost
    more than the pipeline itself on a 128x128x24 study).  Exclusive while held, so host threads never
    share one; at most _BATCH_POOL_KEEP idle batches per shape stay allocated (the rest are closed)."""

    def __init__(self, R, C, Z, n=1, device=0):
        self.key = (int(device), int(R), int(C), int(Z), int(n))

    def __enter__(self):
        with _lock:
            idle = _batch_pool.get(self.key)
            self.b = idle.pop() if idle else None
        if self.b is None or self.b.h is None:
            self.b = Batch(*self.key[1:], device=self.key[0])
        return self.b

    def __exit__(self, exc_type, exc, tb):
        b = self.b
        if exc_type is not None:   # a failed call may have left the batch in any state
            b.close()
            return False
        with _lock:
            idle = _batch_pool.setdefault(self.key, [])
            if len(idle) < _BATCH_POOL_KEEP:
                idle.append(b)
                return False
        b.close()
        return False


class Pipe:
    """Host-to-host pipeline (vh_pipe): n host-resident studies streamed through `slots` device
    batches of `sub` volumes, transfers of one sub-batch overlapping the compute of another."""

    def __init__(self, R, C, Z, sub, slots=3, device=0):
        self.ctx = context(device)
        self.L = self.ctx.L
        self.vshape = (int(R), int(C), int(Z))
        h = _P()
        self.ctx.check(self.L.vh_pipe_create(self.ctx.h, R, C, Z, sub, slots, ct.byref(h)),
                       "vh_pipe_create")
        self.h = h
        _live.add(self)

    def close(self):
        if getattr(self, "h", None):
            self.L.vh_pipe_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self, hp, mask, opts: RunOpts, n4=True, maps=True, out=None):
        """Returns (n4, defect, border, lb, results) host arrays for all len(hp) studies; `out`
        may pass preallocated (n4, defect, border, lb) arrays."""
        h = np.ascontiguousarray(hp, dtype=np.float32)
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        n = h.shape[0]
        if h.shape[1:] != self.vshape or m.shape != h.shape:
            raise ValueError(f"pipe expects (n,) + {self.vshape}")
        if out is None:
            out = (empty_aligned(h.shape, np.float32) if n4 else None,
                   empty_aligned(h.shape, np.uint8) if maps else None,
                   empty_aligned(h.shape, np.uint8) if maps else None,
                   empty_aligned(h.shape, np.uint8) if maps else None)
        res = (VdpResult * n)()
        self.ctx.check(self.L.vh_pipe_run(self.h, _ptr(h), _ptr(m), n, ct.byref(opts),
                                          *[_ptr(a) for a in out], ct.cast(res, ct.c_void_p)),
                       "vh_pipe_run")
        return (*out, list(res))

    def stats(self):
        """(peak bytes of caller memory pinned in place, caller ranges staged instead) of the last
        run (vh_pipe_stats)."""
        pk, st = ct.c_int64(), ct.c_int64()
        self.ctx.check(self.L.vh_pipe_stats(self.h, ct.byref(pk), ct.byref(st)), "vh_pipe_stats")
        return int(pk.value), int(st.value)


def comm_unique_id() -> bytes:
    buf = np.zeros(COMM_ID_BYTES, np.uint8)
    rc = lib().vh_comm_unique_id(_ptr(buf))
    if rc != VH_OK:
        raise VentHipError("ncclGetUniqueId failed")
    return buf.tobytes()


def comm_init(nranks: int, rank: int, uid: bytes, device=0):
    c = context(device)
    buf = np.frombuffer(uid, np.uint8).copy()
    c.check(c.L.vh_comm_init(c.h, nranks, rank, _ptr(buf)), "vh_comm_init")


def comm_info(device=0):
    """(ranks, rank) of the context's RCCL communicator as RCCL reports them (vh_comm_info)."""
    c = context(device)
    n, r = ct.c_int(0), ct.c_int(-1)
    c.check(c.L.vh_comm_info(c.h, ct.byref(n), ct.byref(r)), "vh_comm_info")
    return n.value, r.value


def comm_destroy(device=0):
    """Releases the context's RCCL communicator (vh_comm_destroy)."""
    c = context(device)
    c.L.vh_comm_destroy(c.h)
