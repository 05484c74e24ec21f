"""GPU: the cluster index of a device-resident batch (vh_batch_ci / Batch.ci) against the CPU oracle.
Everything compared is an integer (shells, counts, status) or a product of two float64 values the
oracle forms the same way (radii[shell] * min(vox)), so every comparison is exact."""
import ctypes as ct
import functools

import numpy as np
import pytest

from oracle import native, vdp_oracle as O
from vent_analysis_amd import _lib
from vent_analysis_amd.sphere import compact_table_for
from vent_analysis_amd.synth import synth_batch

pytestmark = pytest.mark.gpu

VOX = (1.5, 1.5, 10.0)


@pytest.fixture(autouse=True, params=[None, "2"], ids=["auto", "form2"])
def ci_form(request, monkeypatch):
    """Every test runs under auto (k_ci_walk at these batch sizes) and with the batch form forced."""
    if request.param is None:
        monkeypatch.delenv("VH_CI_FORM", raising=False)
    else:
        monkeypatch.setenv("VH_CI_FORM", request.param)


def oracle_ci(d, Rmax, vox=VOX):
    """(shell int16, map f64, scalar, status) of one study as download_ci reports them; shell and
    map are None where the oracle raises (the saturated study)."""
    d = np.asarray(d) != 0
    if not d.any():
        return np.full(d.shape, -1, np.int16), np.zeros(d.shape), np.nan, _lib.VH_ERR_EMPTY
    table = compact_table_for(vox, Rmax, d.shape)
    try:
        ref, shell = native.ci(d, table, vox)
    except ValueError:
        return None, None, np.nan, _lib.VH_ERR_MAXRADIUS
    return shell.astype(np.int16), ref, O.ci_scalar(ref[d]), _lib.VH_OK


def batch_ci(ds, Rmax, maps="shell", B=None, vox=VOX):
    """Batch.ci of the maps ds on a fresh batch (or on B) -> download_ci's tuple and the radii."""
    ds = np.ascontiguousarray(ds, dtype=np.uint8)
    own = B is None
    if own:
        B = _lib.Batch(*ds.shape[1:], ds.shape[0])
    B.upload_defect(ds)
    B.ci(vox, Rmax)
    out = B.download_ci(maps=maps)
    radii = B.ci_radii
    if own:
        B.close()
    return out, radii


def assert_equals_oracle(got, radii, refs, minvox=1.5):
    sh, sc, status = got
    assert sh.dtype == np.int16 and sc.dtype == np.float64 and status.dtype == np.int32
    for q, (rsh, rmap, rsc, rst) in enumerate(refs):
        assert status[q] == rst, (q, status[q], rst)
        if rst != _lib.VH_OK:
            assert np.isnan(sc[q]), (q, sc[q])
        else:
            assert sc[q] == rsc, (q, sc[q], rsc)
        if rsh is not None:
            assert np.array_equal(sh[q], rsh), q
            assert np.array_equal(_lib.ci_expand(sh[q], radii, minvox), rmap), q


def blobs(shape, seed, n=7, thin=True):
    """A blob study built as in test_gpu_parity.test_ci_vs_oracle_random_blobs."""
    rng = np.random.default_rng(seed)
    i, j, k = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    d = np.zeros(shape, bool)
    for _ in range(n):
        c = [rng.uniform(-0.1, 1.1) * s for s in shape]
        r = rng.uniform(3, 12)
        d |= (i - c[0]) ** 2 + (j - c[1]) ** 2 + ((k - c[2]) * 3) ** 2 <= r * r
    if thin:
        d &= rng.random(shape) > 0.15
    return d.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def mixed_case():
    """Seven studies of shape (41, 37, 9) -- V is no multiple of 32 -- at Rmax 12: a random map, an
    empty one, a saturated one and maps of 1, 15, 16 and 17 voxels (one wave's worth of a workgroup's
    16 and its neighbours)."""
    shape = (41, 37, 9)
    ds = [(np.random.default_rng(7).random(shape) < 0.2).astype(np.uint8),
          np.zeros(shape, np.uint8), np.ones(shape, np.uint8)]
    rng = np.random.default_rng(8)
    for n in (1, 15, 16, 17):
        d = np.zeros(int(np.prod(shape)), np.uint8)
        d[rng.choice(d.size, n, replace=False)] = 1
        ds.append(d.reshape(shape))
    ds = np.stack(ds)
    refs = [oracle_ci(d, 12) for d in ds]
    for a in (ds, *[x for r in refs for x in r[:2] if x is not None]):
        a.setflags(write=False)
    return ds, refs


@functools.lru_cache(maxsize=None)
def deep_case():
    """Two 128x128x24 studies at Rmax 50.  The solid ellipsoid has 13 749 defect voxels (more than
    512 x 16: k_ci_walk strides), 7 131 walks past table row 8 192 and 2 425 past boundary 1 024:
    rows and boundaries beyond the LDS-resident head.  The second is a blob study."""
    shape = (128, 128, 24)
    i, j, k = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    ell = ((i - 64) ** 2 + (j - 64) ** 2 + ((k - 12) * 10 / 1.5) ** 2 <= 28 ** 2).astype(np.uint8)
    assert int(ell.sum()) == 13749
    ds = np.stack([ell, blobs(shape, 4)])
    refs = [oracle_ci(d, 50) for d in ds]
    for a in (ds, *[x for r in refs for x in r[:2]]):
        a.setflags(write=False)
    return ds, refs


@pytest.mark.parametrize("do_n4", [False, True], ids=["identity", "n4"])
@pytest.mark.parametrize("shape,nb,seed", [((64, 64, 16), 4, 20), ((96, 112, 20), 3, 10)])
def test_ci_after_a_real_run(shape, nb, seed, do_n4):
    """Batch.run then Batch.ci: the CI of each study's resident defect map equals the oracle's CI of
    the downloaded map (shells, expanded map, scalar, status), and the run's own results are the
    same after the CI as before it."""
    hp, mk = synth_batch(*shape, nb, base_seed=seed)
    B = _lib.Batch(*shape, nb)
    B.upload(hp, mk)
    B.run(B.options(do_n4=do_n4, vox=VOX))
    before = B.download(n4=True)
    B.ci(VOX, 50)
    got = B.download_ci(maps="shell")
    after = B.download(n4=True)
    radii = B.ci_radii
    B.close()
    refs = [oracle_ci(before[1][q], 50) for q in range(nb)]
    if not do_n4:   # the oracle chain gives 822 - 3 165 defect voxels per study here, all walkable
        assert all(r[3] == _lib.VH_OK for r in refs)
    assert_equals_oracle(got, radii, refs)
    for a, b in zip(before[:4], after[:4]):
        assert np.array_equal(a, b)
    for ra, rb in zip(before[4], after[4]):
        assert bytes(ra) == bytes(rb)


def test_mixed_status_in_one_batch():
    """An empty study and a saturated one set their own status (scalar NaN) and leave the other
    five studies' results exact; nothing raises."""
    ds, refs = mixed_case()
    assert [r[3] for r in refs] == [_lib.VH_OK, _lib.VH_ERR_EMPTY, _lib.VH_ERR_MAXRADIUS] + [_lib.VH_OK] * 4
    got, radii = batch_ci(ds, 12)
    assert_equals_oracle(got, radii, refs)
    assert np.all(got[0][1] == -1)           # empty: -1 everywhere
    assert np.any(got[0][2] == -1)           # saturated: some voxel reached the last radius


def test_walks_past_the_lds_resident_table_head():
    ds, refs = deep_case()
    got, radii = batch_ci(ds, 50)
    assert_equals_oracle(got, radii, refs)


def test_bitmap_too_large_for_lds():
    """256x256x24: the study's bitmap (192 KiB) stays in L2."""
    shape = (256, 256, 24)
    ds = np.stack([blobs(shape, s, n=5) for s in (1, 2)])
    refs = [oracle_ci(d, 50) for d in ds]
    got, radii = batch_ci(ds, 50)
    assert_equals_oracle(got, radii, refs)


@pytest.mark.parametrize("case,Rmax", [(mixed_case, 12), (deep_case, 50)], ids=["mixed", "deep"])
def test_forms_agree(case, Rmax, monkeypatch):
    """VH_CI_FORM=1 (k_ci_walk over the resident batch) and =2 (the batch form): identical shells,
    scalars and status, both equal to the oracle's."""
    ds, refs = case()
    out = {}
    for form in ("1", "2"):
        monkeypatch.setenv("VH_CI_FORM", form)
        out[form], radii = batch_ci(ds, Rmax)
        assert_equals_oracle(out[form], radii, refs)
    for a, b in zip(out["1"], out["2"]):
        assert np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("order", [(0, 1), (1, 0)], ids=["small-then-large", "large-then-small"])
def test_batch_reuse_across_maps_and_tables(order):
    """One Batch, two sets of maps and two tables of different shell counts (Rmax 12, then 50, and
    the other way round): each result equals a fresh batch's, and the f64 download equals ci_expand
    of the shell download."""
    shape = (41, 37, 9)
    sets = [(np.stack([blobs(shape, 21), blobs(shape, 22, thin=False)]), 12),
            (np.stack([blobs(shape, 23, n=3), np.zeros(shape, np.uint8)]), 50)]
    B = _lib.Batch(*shape, 2)
    for s in order:
        ds, Rmax = sets[s]
        fresh, radii = batch_ci(ds, Rmax)
        got, radii_b = batch_ci(ds, Rmax, B=B)
        assert radii_b is radii
        for a, b in zip(fresh, got):
            assert np.array_equal(a, b, equal_nan=True)
        f64, sc, st = B.download_ci(maps="f64")
        assert np.array_equal(f64, _lib.ci_expand(got[0], radii, 1.5))
        assert np.array_equal(sc, got[1], equal_nan=True) and np.array_equal(st, got[2])
        none, sc, st = B.download_ci(maps=None)
        assert none is None and np.array_equal(sc, got[1], equal_nan=True)
        assert_equals_oracle(got, radii, [oracle_ci(d, Rmax) for d in ds])
    B.close()


def test_table_destroyed_right_after_the_enqueue():
    """vh_ci_table_destroy straight after vh_batch_ci returns waits for the enqueued walk: the
    results are the oracle's."""
    ds, refs = deep_case()
    B = _lib.Batch(*ds.shape[1:], ds.shape[0])
    B.upload_defect(ds)
    c = B.ctx
    with c.ci_lock:
        B.ci(VOX, 50)
        table = compact_table_for(VOX, 50, ds.shape[1:])
        key = (table.key, ds.shape[1], ds.shape[2])
        _, th = c.ci_tables.pop(key)
        assert c.L.vh_ci_table_destroy(th) == _lib.VH_OK
    got = B.download_ci(maps="shell")
    f64, _, _ = B.download_ci(maps="f64")   # the radii are the batch's own copy by now
    radii = B.ci_radii
    B.close()
    assert_equals_oracle(got, radii, refs)
    assert np.array_equal(f64, _lib.ci_expand(got[0], radii, 1.5))


def test_batch_ci_argument_errors():
    shape = (41, 37, 9)
    B = _lib.Batch(*shape, 1)
    with pytest.raises(ValueError):
        B.download_ci()                      # before any ci()
    with pytest.raises(ValueError):
        B.ci(VOX, 12)                        # no defect maps resident
    B.upload_defect(np.zeros((1,) + shape, np.uint8))
    c = B.ctx
    with c.ci_lock:   # a device table of another R
        th = c.ci_table(compact_table_for(VOX, 12, (40, 37, 9)), 40, 37)
        assert c.L.vh_batch_ci(B.h, th, ct.c_double(1.5)) == _lib.VH_ERR_ARG
    assert c.L.vh_batch_ci(B.h, None, ct.c_double(1.5)) == _lib.VH_ERR_ARG
    B.ci(VOX, 12)
    _, sc, st = B.download_ci(maps=None)
    assert st[0] == _lib.VH_ERR_EMPTY and np.isnan(sc[0])
    B.close()


def test_ci_workspace_grows_on_one_batch():
    """One resident batch, the same maps under a table of few shells (Rmax 12) and then one of more
    (Rmax 50): the shell histograms and the batch's copy of the radii are freed and allocated again.
    Scalars, status and the int16 map equal those of a fresh batch given only the second table."""
    shape = (40, 36, 9)
    ds = np.stack([blobs(shape, 31), blobs(shape, 32, n=3)])
    B = _lib.Batch(*shape, 2)
    try:
        small, radii_small = batch_ci(ds, 12, B=B)
        got, radii = batch_ci(ds, 50, B=B)
    finally:
        B.close()
    assert len(radii) > len(radii_small)
    fresh, radii_f = batch_ci(ds, 50)
    assert radii_f is radii
    for a, b in zip(fresh, got):
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)
    assert np.all(got[2] == _lib.VH_OK)
