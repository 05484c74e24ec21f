"""The run option ``thresh`` off 0.6: the mean-anchored defect map N4 / mean < thresh (float32, strict)
through Batch.run, vh_vdp (_lib.vdp), vh_pipe (Pipe.run), Batch.select_defect and vh_defect_map,
against oracle.vdp_oracle.calculate_vdp and defect_select_ref.reference at the same threshold.  The
threshold moves the defect map, its border, VDP and the defect count alone: the LB map, VDP_lb, the
k-means clusters, p99 and the anchor are those of the thresh = 0.6 run.

The volumes are defect_select_ref.field's (a smooth noisy field whose defect map differs at each
threshold; synth_volume's clean-zero defects give one map below the bulk), three studies per shape,
with do_n4 = False throughout."""
import functools

import numpy as np
import pytest

from oracle import vdp_oracle as O
from vent_analysis_amd import _lib

import defect_select_ref as D

F32 = np.float32
VOX = D.VOX
SHAPES = [(37, 45, 7), (50, 33, 1)]
THRESH = [0.45, 0.75, 1.0, 1.5]
N = 3


@functools.lru_cache(maxsize=None)
def studies(shape):
    hp, mk = (np.stack(a) for a in zip(*(D.field(shape, seed) for seed in (1, 2, 3))))
    hp.setflags(write=False)
    mk.setflags(write=False)
    return hp, mk


@functools.lru_cache(maxsize=None)
def oracle(shape, thresh):
    """[calculate_vdp(study, thresh)] of studies(shape)."""
    hp, mk = studies(shape)
    return [O.calculate_vdp(hp[q], mk[q].astype(np.float64), VOX, thresh=thresh) for q in range(N)]


def batch_run(shape, thresh):
    hp, mk = studies(shape)
    B = _lib.Batch(*shape, N)
    B.upload(hp, mk)
    B.run(B.options(do_n4=False, vox=VOX, thresh=thresh))
    return B


@functools.lru_cache(maxsize=None)
def at_default(shape):
    """(defect, border, lb, results) of the thresh = 0.6 run of the batch."""
    B = batch_run(shape, 0.6)
    out = B.download()[1:]
    B.close()
    return out


def assert_maps(got, shape, thresh, tag):
    """(defect, border, lb, results) against the oracle at ``thresh`` and the thresh = 0.6 run."""
    d, bo, lb, res = got
    _, mk = studies(shape)
    _, _, lb6, res6 = at_default(shape)
    for q, o in enumerate(oracle(shape, thresh)):
        assert np.array_equal(d[q], o["defectArray"]), (tag, q)
        assert np.array_equal(bo[q] == 1, o["defectBorder"]), (tag, q)
        assert res[q].vdp == o["VDP"], (tag, q, res[q].vdp, o["VDP"])
        assert res[q].n_defect == int(o["defectArray"].sum()), (tag, q)
        assert res[q].n_mask == int(mk[q].sum())
        # what the threshold does not reach
        assert np.array_equal(lb[q], o["defectArrayLB"]) and np.array_equal(lb[q], lb6[q]), (tag, q)
        assert res[q].vdp_lb == o["VDP_lb"] == res6[q].vdp_lb, (tag, q)
        assert F32(res[q].p99) == o["p99"] and res[q].p99 == res6[q].p99, (tag, q)
        assert F32(res[q].mean_anchor) == o["mean_anchor"] and res[q].mean_anchor == res6[q].mean_anchor
        for name in ("n_lb12", "n_km0", "vdp_km", "lung_volume"):
            assert getattr(res[q], name) == getattr(res6[q], name), (tag, q, name)
        assert list(res[q].km_centres) == list(res6[q].km_centres), (tag, q)


def test_the_thresholds_give_different_maps():
    """(host) The cases are not vacuous: on every study the four thresholds and 0.6 give five
    different defect counts in the oracle."""
    for shape in SHAPES:
        counts = [[int(o["defectArray"].sum()) for o in oracle(shape, t)] for t in [0.6] + THRESH]
        for q in range(N):
            assert len({c[q] for c in counts}) == 5, (shape, q, counts)


@pytest.mark.gpu
@pytest.mark.parametrize("thresh", THRESH)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_batch_run(shape, thresh):
    B = batch_run(shape, thresh)
    try:
        got = B.download()[1:]
        assert_maps(got, shape, thresh, "batch")
        hp, mk = studies(shape)
        refs = [D.reference(hp[q], mk[q], thresh=thresh) for q in range(N)]
        for medfilt in (0, 1, 2):   # the selection takes the run's threshold
            B.select_defect("mean", medfilt)
            d, bo, cnt = B.download_defect()
            for q, r in enumerate(refs):
                rd, rbo = D.filtered(r["raw"]["mean"], medfilt)
                assert np.array_equal(d[q], rd) and np.array_equal(bo[q], rbo), (medfilt, q)
                assert cnt[q] == int(rd.sum()), (medfilt, q)
        B.select_defect("mean", 1)   # the run's own map again
        d, bo, cnt = B.download_defect()
        assert np.array_equal(d, got[0]) and np.array_equal(bo, got[1])
        assert list(cnt) == [r.n_defect for r in got[3]]
    finally:
        B.close()


@pytest.mark.gpu
@pytest.mark.parametrize("thresh", THRESH)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_host_entry_points(shape, thresh):
    """vh_vdp and vh_defect_map with the threshold as their argument."""
    hp, mk = studies(shape)
    assert_maps(_lib.vdp(hp, mk, VOX, hp=hp, thresh=thresh), shape, thresh, "vh_vdp")
    for medfilt in (0, 1, 2):
        d, bo, cnt = _lib.defect_map(hp, mk, "mean", medfilt, thresh=thresh)
        for q in range(N):
            rd, rbo = D.filtered(D.reference(hp[q], mk[q], thresh=thresh)["raw"]["mean"], medfilt)
            assert np.array_equal(d[q], rd) and np.array_equal(bo[q], rbo), (medfilt, q)
            assert cnt[q] == int(rd.sum()), (medfilt, q)


@pytest.mark.gpu
@pytest.mark.parametrize("thresh", THRESH)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_pipe_run(shape, thresh):
    """vh_pipe, three studies in sub-batches of two (a ragged last one), two slots."""
    hp, mk = studies(shape)
    pipe = _lib.Pipe(*shape, 2, slots=2)
    try:
        got = pipe.run(hp, mk, _lib.Batch.options(do_n4=False, vox=VOX, thresh=thresh), n4=False)
    finally:
        pipe.close()
    assert_maps(got[1:], shape, thresh, "pipe")


# ---- the comparison is a strict float32 < -------------------------------------------------------------
A_BLOCK = (slice(8, 11), slice(8, 12), 3)     # 12 voxels at exactly 1.0
B_BLOCK = (slice(20, 23), slice(20, 24), 3)   # 12 voxels one float32 below 1.0
BELOW = np.nextafter(F32(1.0), F32(0.0))


@functools.lru_cache(maxsize=None)
def equality_case():
    """A 37x45x7 study whose mean-anchored value is exactly the threshold 0.5 on one group of voxels
    and one float32 below it on another.  The map divides by the float32 mean of the masked values
    (calculate_vdp; the 99th percentile anchors the LB map, not this one), so the mean is what is put
    at exactly 2.0: every masked voxel 2.0 but 12 at 1.0 (A), 12 at nextafter(1, 0) (B) and one at 26.0,
    which balances the 24 (the float32 sums are of small integers but for B's 12 * 2^-24, far below
    half an ulp of the mean).  The int(n * 0.99)-th sorted value is 2.0 as well.  A and B are 3x4
    blocks of one slice, 9 columns apart: no 3x3 window holds voxels of both, so the median keeps
    them apart."""
    _, M = D.field((37, 45, 7), 1)
    X = np.where(M > 0, 2.0, 0.5).astype(F32)
    assert M[A_BLOCK].all() and M[B_BLOCK].all() and M[18, 30, 5]
    X[A_BLOCK] = 1.0
    X[B_BLOCK] = BELOW
    X[18, 30, 5] = 26.0
    X.setflags(write=False)
    M.setflags(write=False)
    return X, M


def assert_equality_maps(raw, filt, tag):
    """raw / filt: the medfilt 0 / 1 maps of equality_case() at thresh 0.5."""
    X, M = equality_case()
    assert raw[B_BLOCK].all() and not raw[A_BLOCK].any(), tag
    assert int(raw.sum()) == 12, (tag, int(raw.sum()))
    assert filt[21, 21, 3] == 1 and filt[21, 22, 3] == 1 and not filt[A_BLOCK].any(), tag
    r = D.reference(X, M, thresh=0.5)["raw"]["mean"]
    assert np.array_equal(raw, r), tag
    assert np.array_equal(filt, D.filtered(r, 1)[0]), tag


def test_equality_case_on_the_oracle():
    """(host) The construction does what it says in the numpy oracle: mean and p99 exactly 2.0, A at
    exactly the threshold and outside the map, B inside, before and after the median; a <= in place
    of < would take A in."""
    X, M = equality_case()
    sig = np.sort(X[M > 0], kind="stable")
    m = O.mean_f32(sig)
    assert m == F32(2.0) and sig[int(len(sig) * .99)] == F32(2.0)
    assert F32(F32(1.0) / m) == F32(0.5) and F32(BELOW / m) < F32(0.5)
    o = O.calculate_vdp(X, M.astype(np.float64), VOX, thresh=0.5)
    raw = D.reference(X, M, thresh=0.5)["raw"]["mean"]
    assert_equality_maps(raw, o["defectArray"], "oracle")
    loose = ((X / m).astype(F32) <= F32(0.5)) & (M > 0)
    assert loose[A_BLOCK].all() and int(loose.sum()) == 24


@pytest.mark.gpu
def test_the_comparison_is_strict_in_float32():
    X, M = equality_case()
    o = O.calculate_vdp(X, M.astype(np.float64), VOX, thresh=0.5)
    B = _lib.Batch(37, 45, 7, 1)
    try:
        B.upload(X[None], M[None])
        B.run(B.options(do_n4=False, vox=VOX, thresh=0.5))
        _, d, bo, _, res = B.download()
        assert F32(res[0].mean_anchor) == F32(2.0) and F32(res[0].p99) == F32(2.0)
        assert np.array_equal(d[0], o["defectArray"]) and np.array_equal(bo[0] == 1, o["defectBorder"])
        assert res[0].vdp == o["VDP"] and res[0].n_defect == int(o["defectArray"].sum())
        B.select_defect("mean", 0)
        raw = B.download_defect()[0]
        assert_equality_maps(raw[0], d[0], "batch")
    finally:
        B.close()
    dv, _, _, resv = _lib.vdp(X, M, VOX, hp=X, thresh=0.5)
    rawv = _lib.defect_map(X, M, "mean", 0, thresh=0.5)[0]
    assert resv[0].n_defect == res[0].n_defect
    assert_equality_maps(rawv[0], dv[0], "host entry points")
