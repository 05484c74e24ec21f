"""The numpy reference of the fine registration (include/vent_hip.h, "fine registration"): the candidate
formula in float64, the resampler's tables and three axis passes (resample_ref) shared between the
candidates as the spec's nested sum allows, the skip rule, the codes by the source maximum, the joint
histogram and the mutual information (register_ref), and the pick; and the seeded phantom the host and GPU
tests share.  Every count is an integer; only mi is floating point."""
import functools

import numpy as np

import register_ref as G
import resample_ref as S

LEVELS = G.LEVELS


# ---- candidate lists and the pick ---------------------------------------------------------------------
def axis_candidates(base, n_dst, factors, shifts):
    """float64 [nf * ns][2]: every operation a separately rounded double, in the order of the spec."""
    s0, o0 = np.float64(base[0]), np.float64(base[1])
    c = (np.float64(n_dst) - np.float64(1.0)) / np.float64(2.0)
    out = np.zeros((len(factors) * len(shifts), 2), np.float64)
    for fi, f in enumerate(factors):
        for si, d in enumerate(shifts):
            f, d = np.float64(f), np.float64(d)
            scale = s0 * f
            one_f = np.float64(1.0) - f
            lever = c * one_f
            moved = lever + d
            in_src = s0 * moved
            out[fi * len(shifts) + si] = (scale, o0 + in_src)
    return out


def candidates(count):
    """Every (kr, kc, kz) in index order: kz slowest, then kr, then kc."""
    Kr, Kc, Kz = count
    return [(kr, kc, kz) for kz in range(Kz) for kr in range(Kr) for kc in range(Kc)]


def middle(count):
    return tuple((int(k) - 1) // 2 for k in count)


def pick(score, count, home=None):
    """The best (kr, kc, kz) of one study's scores: the largest, then the smallest L1 distance from home,
    then the lowest index; a NaN never wins, and nothing but NaN gives home."""
    home = middle(count) if home is None else tuple(int(v) for v in home)
    best, key = home, None
    for i, (k, v) in enumerate(zip(candidates(count), np.asarray(score, np.float64).reshape(-1))):
        if np.isnan(v):
            continue
        q = (-float(v), sum(abs(a - h) for a, h in zip(k, home)), i)
        if key is None or q < key:
            best, key = k, q
    return best


# ---- the values and the histograms of one study --------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _taps(n_src, n_dst, scale, offset):
    return S.taps(n_src, n_dst, scale, offset)


def values(src, dst_shape, lists):
    """Yields (kr, kc, kz, Q float32 dst_shape, counted bool dst_shape) in index order: Q the resampling of
    src under (r[kr], c[kc], z[kz]) -- the z-pass shared by a kz, the c-pass by a (kz, kc), which the exactly
    separable nested sum allows -- and counted false where an axis has no tap."""
    src = np.asarray(src, np.float32)
    rl, cl, zl = lists
    for kz, mz in enumerate(zl):
        tz = _taps(src.shape[2], dst_shape[2], float(mz[0]), float(mz[1]))
        A = S._axis_pass(src, tz, 2)
        per_c = []
        for mc in cl:
            tc = _taps(src.shape[1], dst_shape[1], float(mc[0]), float(mc[1]))
            per_c.append((tc, S._axis_pass(A, tc, 1)))
        for kr, mr in enumerate(rl):
            tr = _taps(src.shape[0], dst_shape[0], float(mr[0]), float(mr[1]))
            for kc, (tc, B) in enumerate(per_c):
                Q = S._axis_pass(B, tr, 0)
                counted = (tr[1] > 0)[:, None, None] & (tc[1] > 0)[None, :, None] & (tz[1] > 0)[None, None, :]
                yield kr, kc, kz, Q, counted


def value_nested(src, dst_shape, m):
    """One candidate a voxel at a time, exactly as the spec writes it (tiny cases only)."""
    (_, kr, _), (_, kc, _), (_, kz, _) = S.tables(np.shape(src), dst_shape, m)
    counted = (kr > 0)[:, None, None] & (kc > 0)[None, :, None] & (kz > 0)[None, None, :]
    return S.resample_nested(src, dst_shape, m), counted


def source_codes(Q, smax):
    """uint8 codes of Q by the study's one scale 256.0f / smax, 255 where Q is not finite or < 0."""
    Q = np.asarray(Q, np.float32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        valid = np.isfinite(Q) & (Q >= 0)
        scale = np.float32(256.0) / np.float32(smax)
        prod = (np.where(valid, Q, np.float32(0)) * scale).astype(np.float32)
        small = prod < np.float32(255.0)
        bins = np.where(small, np.where(small, prod, 0).astype(np.int64), 255)
    return np.where(valid, bins >> 3, G.INVALID).astype(np.uint8)


def joint(cq, cx, counted):
    a = cq.astype(np.int64).reshape(-1)
    b = cx.astype(np.int64).reshape(-1)
    ok = (a != G.INVALID) & (b != G.INVALID) & counted.reshape(-1)
    return np.bincount(a[ok] * LEVELS + b[ok], minlength=LEVELS * LEVELS).astype(np.uint32).reshape(LEVELS, LEVELS)


def gap(score):
    return G.gap(score)


def reference_of(src, X, lists, home=None):
    """src [n][Rs][Cs][Zs], X [n][R][C][Z], lists [n] of (r, c, z) lists -> (hist uint32 [n][nc][32][32],
    score float64 [n][nc], best [n] of (kr, kc, kz), status [n])."""
    n = len(src)
    dst_shape = X.shape[1:]
    count = tuple(len(l) for l in lists[0])
    nc = count[0] * count[1] * count[2]
    hist = np.zeros((n, nc, LEVELS, LEVELS), np.uint32)
    score = np.zeros((n, nc), np.float64)
    best, status = [], []
    h = middle(count) if home is None else tuple(home)
    for q in range(n):
        smax, cx = G.image_max(src[q]), G.codes(X[q])
        if not smax > 0 or cx is None:
            score[q] = np.nan
            best.append(h)
            status.append(1)
            continue
        for kr, kc, kz, Q, counted in values(src[q], dst_shape, lists[q]):
            i = (kz * count[0] + kr) * count[1] + kc
            hist[q, i] = joint(source_codes(Q, smax), cx, counted)
            score[q, i] = G.mi(hist[q, i])
        best.append(pick(score[q], count, h))
        status.append(0)
    return hist, score, best, np.asarray(status, np.int32)


# ---- the phantom ---------------------------------------------------------------------------------------
def xenon_of(src, dst_shape, m, seed, kind=0):
    """The xenon float32 of dst_shape derived from the source resampled through the map m: bright where
    the proton is dark inside the body, X = rician(where(body, clip(130 - Pres, 0) * 0.7 * vent, 0), 3)."""
    rng = np.random.default_rng(seed)
    with np.errstate(invalid="ignore"):
        pres = np.nan_to_num(S.resample(src, dst_shape, m).astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0)
    body, _, vent = G._anatomy(dst_shape, (0, 0, 0))
    x = G._rician(rng, np.where(body, np.clip(130.0 - pres, 0.0, None) * 0.7 * vent, 0.0), 3.0)
    if kind == 1:
        x = np.where(body, x, 0.0)
    return x


def _salt(rng, img):
    at = rng.random(img.shape)
    img[at < 0.004] = np.nan
    img[(at >= 0.004) & (at < 0.006)] = np.inf
    img[(at >= 0.006) & (at < 0.008)] = -np.inf
    img[(at >= 0.008) & (at < 0.014)] *= -1.0


def _lists(base, n_dst, factors, shifts, zfactors, zshifts):
    return [axis_candidates(base[a], n_dst[a], zfactors if a == 2 else factors, zshifts if a == 2 else shifts)
            for a in range(3)]


def _pairs(*p):
    return np.asarray(p, np.float64)


def _case_lists(case, q):
    """The (r, c, z) lists of study q of a case."""
    if case == 1:     # scale near 2 with fractional offsets; each study around a base of its own
        base = [(2.0, 1.0 + 0.13 * q), (2.0, 1.0 - 0.21 * q), (1.0, 0.05 * q)]
        return _lists(base, (41, 37, 9), (0.94, 1.0, 1.06), (-0.5, 0.0, 0.5), (1.0,), (-0.5, 0.0, 0.5))
    if case == 2:     # upsampling on every axis; Kz = 1
        base = [(0.5, 0.1 * q), (0.5, -0.07 * q), (0.5, 0.0)]
        return _lists(base, (41, 37, 9), (0.9, 1.0, 1.1), (-0.5, 0.0, 0.5), (1.0,), (0.0,))
    if case == 3:     # both list limits; mixed scales; part of the destination outside the source; > 2 z-taps
        r = _pairs((1.7, -0.4), (1.7, -7.25), (1.55, 2.0 + q))
        c = _pairs(*[(0.6, o) for o in (-3.0, -1.2, 0.3, 0.8, 2.5, 6.0, 11.0, 18.5, 25.0)],
                   *[(1.05, o) for o in (-2.0, -0.5, 0.0, 0.4, 1.0, 3.0, 7.0, 12.0)])
        z = _pairs((1.3, 0.2), (1.3, -2.0), (1.3, 4.0), (1.0, 0.0), (1.25, 0.7))
        return [r, c, z]
    if case == 4:     # eight row taps; the r list chunked under a small budget
        return [_pairs((3.9, 0.0), (4.0, -3.0 + q)), _pairs((1.0, 0.0), (1.0, 0.5)), _pairs((1.0, 0.0))]
    if case == 5:     # a one-voxel source, a one-slice batch: a single candidate
        return [_pairs((1.0, 0.0)), _pairs((1.0, 0.0)), _pairs((1.0, 0.0))]
    if case == 6:     # ... and 3 x 3 x 1 of them
        return [_pairs((1.0, -5.5), (0.25, -1.0), (4.0, -20.0)), _pairs((1.0, -4.5), (0.25, -1.0), (0.5, -2.0)),
                _pairs((1.0, 0.3))]
    if case == 7:     # the bench shape
        base = [(2.0, 0.5 + 0.25 * q), (2.0, 0.5 - 0.25 * q), (1.0, 0.0)]
        return _lists(base, (128, 128, 24), (0.97, 1.0, 1.03), (0.0,), (1.0,), (0.0,))
    raise KeyError(case)


# case -> (source shape, destination shape, studies, the planted (kr, kc, kz) of studies 0.. or None)
CASES = {
    1: ((83, 75, 9), (41, 37, 9), 4, [(1, 7, 2), (6, 2, 0), (8, 3, 1)]),
    2: ((21, 19, 5), (41, 37, 9), 4, None),
    3: ((64, 40, 12), (41, 37, 9), 4, None),
    4: ((160, 37, 9), (41, 37, 9), 4, None),
    5: ((1, 1, 1), (12, 10, 1), 4, None),
    6: ((1, 1, 1), (12, 10, 1), 4, None),
    7: ((256, 256, 24), (128, 128, 24), 2, None),
}
MIN_GAP = 1e-3      # a recovery is asserted only where the reference's best beats its second by this


@functools.lru_cache(maxsize=None)
def batch(case):
    """(source float32 [n][Rs][Cs][Zs], xenon float32 [n][R][C][Z], lists [n] of (r, c, z)), read-only.
    Case 1: studies 0..2 of kinds 0 (noise everywhere), 1 (the background of both images exactly 0) and 2
    (salted with NaN, +-inf and negatives), the xenon derived through the planted candidate; study 3 a
    constant source.  Elsewhere the xenon is derived through the middle candidate."""
    src_shape, dst_shape, n, planted = CASES[case]
    srcs, xs, lists = [], [], []
    for q in range(n):
        seed = 1000 * q + 17 * case + sum(src_shape)
        s = S.study(src_shape, seed)
        L = _case_lists(case, q)
        kind = q if (case == 1 and q < 3) else 0
        k = planted[q] if planted and q < len(planted) else middle([len(l) for l in L])
        m = [L[0][k[0]], L[1][k[1]], L[2][k[2]]]
        if kind == 1:
            s = np.where(G._anatomy(src_shape, (0, 0, 0))[0], s, np.float32(0))
        x = xenon_of(s, dst_shape, m, seed + 1, kind)
        if kind == 2:
            rng = np.random.default_rng(seed + 2)
            s = s.copy()
            _salt(rng, s)
            _salt(rng, x)
        if case == 1 and q == 3:
            s = np.full(src_shape, 7.5, np.float32)
        srcs.append(s.astype(np.float32))
        xs.append(x.astype(np.float32))
        lists.append(L)
    A, X = np.stack(srcs), np.stack(xs)
    A.setflags(write=False)
    X.setflags(write=False)
    return A, X, lists


def axis_maps(lists):
    """[n] of (r, c, z) lists -> the three arrays [n][K][2] a binding takes."""
    return [np.stack([np.asarray(l[a], np.float64) for l in lists]) for a in range(3)]


@functools.lru_cache(maxsize=None)
def reference(case):
    """(hist, score, best, status) of batch(case) with home the middle candidate, read-only."""
    A, X, lists = batch(case)
    hist, score, best, status = reference_of(A, X, lists)
    hist.setflags(write=False)
    score.setflags(write=False)
    return hist, score, best, status
