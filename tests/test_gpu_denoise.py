"""GPU: the denoise option of a resident batch (vh_batch_denoise / Batch.denoise and the layers above
it) against the numpy reference (denoise_ref).  The filter is specified to the last bit: every
comparison of volumes is np.array_equal on float32."""
import functools

import numpy as np
import pytest

from vent_analysis_amd import _lib

import denoise_ref as D

pytestmark = pytest.mark.gpu

F32 = np.float32


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == F32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@functools.lru_cache(maxsize=None)
def resident(shape):
    """One batch of three studies per shape, kept for the parametrised cases (each uploads again:
    denoise replaces the resident HPvent)."""
    return _lib.Batch(*shape, 3)


@pytest.mark.parametrize("rician", (False, True))
@pytest.mark.parametrize("search,patch", D.PARAMS)
@pytest.mark.parametrize("shape", D.SHAPES, ids=str)
def test_denoise_equals_the_reference(shape, search, patch, rician):
    """Three studies with three sigmas (a per-study parameter mix-up shows), the all-zero study
    included; float32 bits."""
    hp, mk = D.batch_inputs(shape), D.batch_masks(shape)
    B = resident(shape)
    B.upload(hp, mk)
    used = B.denoise(D.SIGMAS, D.STRENGTH, search, patch, rician)
    got = B.download_hp()
    assert used.tobytes() == np.asarray(D.SIGMAS, F32).tobytes()
    ref = D.batch_reference(shape, search, patch, rician)
    for q in range(3):
        assert same_bits(got[q], ref[q]), (q, np.abs(got[q] - ref[q]).max(), int((got[q] != ref[q]).sum()))
    assert not got[2].any()   # 0 / 1 = 0, and sqrt is not taken of 0 - bias


def test_denoising_twice_is_the_filter_of_the_filter():
    """The output becomes the resident HPvent: a second call reads it."""
    shape = (41, 37, 9)
    hp, mk = D.batch_inputs(shape), D.batch_masks(shape)
    B = resident(shape)
    B.upload(hp, mk)
    B.denoise(D.SIGMAS, D.STRENGTH, 1, 0)
    B.denoise(D.SIGMAS, D.STRENGTH, 1, 0)
    got = B.download_hp()
    once = D.batch_reference(shape, 1, 0, False)
    for q in range(2):
        assert same_bits(got[q], D.denoise(once[q], D.SIGMAS[q], D.STRENGTH, 1, 0)), q


def within_one_ulp(got, ref):
    """Elementwise: equal, both NaN, or one float32 step apart."""
    got, ref = np.asarray(got, F32), np.asarray(ref, F32)
    nan = np.isnan(ref)
    if not np.array_equal(np.isnan(got), nan):
        return False
    return bool(np.all(np.abs(got[~nan].astype(np.float64) - ref[~nan]) <= np.spacing(np.abs(ref[~nan]))))


@pytest.mark.parametrize("shape", D.SHAPES, ids=str)
def test_noise_sigma(shape):
    """Against the reference within one float32 ulp: the device and numpy sum the doubles in different
    orders, a relative difference of about 1e-12 in S2, which can move the float32 rounding by at most
    one step.  The empty mask (and, at 5 rows, every study: no row inside the FOV band) gives NaN."""
    hp, mk = D.batch_inputs(shape), D.batch_masks(shape)
    B = resident(shape)
    B.upload(hp, mk)
    got = B.noise_sigma()
    ref = np.array([D.noise_sigma(hp[q], mk[q]) for q in range(3)], F32)
    print(shape, got, ref)
    assert got.dtype == F32 and within_one_ulp(got, ref), (got, ref)
    assert np.isnan(got[2])
    assert same_bits(B.download_hp(), hp)                           # the estimate changes no volume
    assert same_bits(_lib.noise_sigma(hp, mk), got)                 # the host-buffer form


def test_sigma_none_uses_the_estimate():
    shape = (64, 64, 24)
    hp, mk = D.batch_inputs(shape)[:2], D.batch_masks(shape)[:2]
    B = _lib.Batch(*shape, 2)
    B.upload(hp, mk)
    est = B.noise_sigma()
    used = B.denoise()           # sigma=None, the defaults: strength 2.0, (3, 1), rician off
    got = B.download_hp()
    B.close()
    assert same_bits(used, est) and np.isfinite(est).all()
    for q in range(2):
        assert same_bits(got[q], D.denoise(hp[q], est[q])), q


def test_sigma_none_refuses_an_undefined_estimate():
    shape = (41, 37, 9)
    hp, mk = D.batch_inputs(shape), D.batch_masks(shape)
    B = resident(shape)
    B.upload(hp, mk)
    with pytest.raises(ValueError):
        B.denoise()              # study 2: an empty mask, NaN
    assert same_bits(B.download_hp(), hp)   # nothing was enqueued


def test_library_argument_errors():
    """The library's own checks (the binding's are bypassed): VH_ERR_ARG, nothing enqueued."""
    import ctypes as ct
    shape = (5, 7, 3)
    hp, mk = D.batch_inputs(shape), D.batch_masks(shape)
    B = resident(shape)
    B.upload(hp, mk)
    ok = np.asarray(D.SIGMAS, F32)
    call = lambda sg, k, s, p: B.L.vh_batch_denoise(B.h, _lib._ptr(sg), ct.c_float(k), s, p, 0)  # noqa: E731
    for sg, k, s, p in ((None, 2.0, 3, 1), (ok, 2.0, 0, 1), (ok, 2.0, 6, 1), (ok, 2.0, 3, -1), (ok, 2.0, 3, 3),
                        (ok, 0.0, 3, 1), (ok, -1.0, 3, 1), (ok, np.inf, 3, 1), (ok, np.nan, 3, 1),
                        (np.array([1, 0, 1], F32), 2.0, 3, 1), (np.array([1, 1, -1], F32), 2.0, 3, 1),
                        (np.array([np.nan, 1, 1], F32), 2.0, 3, 1), (np.array([1, np.inf, 1], F32), 2.0, 3, 1)):
        assert call(sg, k, s, p) == _lib.VH_ERR_ARG, (sg, k, s, p)
    with pytest.raises(ValueError):
        B.ctx.check(call(ok, 2.0, 0, 1), "vh_batch_denoise")
    assert same_bits(B.download_hp(), hp)


def result_bytes(res):
    return [bytes(r) for r in res]


@functools.lru_cache(maxsize=None)
def downstream(do_n4):
    """(41, 37, 9): (a) upload, denoise, run, download; (b) a fresh batch uploaded with the
    reference-denoised volumes, run, download.  With N4 the empty-mask study stays out."""
    shape = (41, 37, 9)
    n = 2 if do_n4 else 3
    hp, mk = D.batch_inputs(shape)[:n], D.batch_masks(shape)[:n]
    ref = D.batch_reference(shape, 3, 1, False)[:n]
    out = []
    for src, dn in ((hp, True), (ref, False)):
        B = _lib.Batch(*shape, n)
        B.upload(src, mk)
        if dn:
            B.denoise(D.SIGMAS[:n], D.STRENGTH, 3, 1)
        B.run(B.options(do_n4=do_n4, vox=D.VOX))
        out.append(B.download(n4=True) + (B.download_hp(),))
        B.close()
    return out, ref


@pytest.mark.parametrize("do_n4", (False, True), ids=("plain", "n4"))
def test_the_next_run_sees_the_denoised_volume(do_n4):
    """N4 (when on), SNR and the VDP chain read the denoised HPvent: every volume, map and scalar
    equals that of a fresh batch uploaded with the reference-denoised volumes."""
    (a, b), ref = downstream(do_n4)
    assert same_bits(a[5], ref) and same_bits(b[5], ref)
    if not do_n4:
        assert same_bits(a[0], ref)          # download(n4=True) without N4: the denoised volume
    assert same_bits(a[0], b[0])
    for k in (1, 2, 3):
        assert np.array_equal(a[k], b[k]), k
    assert result_bytes(a[4]) == result_bytes(b[4])
    assert a[4][0].n_mask > 0 and a[4][0].n_defect >= 0 and np.isfinite(a[4][0].snr)


def test_after_a_run_denoise_puts_the_batch_back_to_uploaded():
    shape = (41, 37, 9)
    hp, mk = D.batch_inputs(shape), D.batch_masks(shape)
    B = _lib.Batch(*shape, 3)
    B.upload(hp, mk)
    B.run(B.options(do_n4=False, vox=D.VOX))
    B.download()
    B.denoise(D.SIGMAS, D.STRENGTH, 1, 0)
    for call in (B.download, B.download_defect, lambda: B.select_defect("mean"), B.distribution, B.overlay,
                 B.montage_layout, B.km_cuts):
        with pytest.raises(ValueError):
            call()
    B.run(B.options(do_n4=False, vox=D.VOX))
    n4 = B.download(n4=True)[0]
    B.close()
    assert same_bits(n4, D.batch_reference(shape, 1, 0, False))


def test_host_buffer_forms_and_class_methods():
    """vh_denoise / vh_noise_sigma on host arrays and Vent_Analysis.denoise / estimate_noise return
    the batch's bits; the class methods leave the object as it was."""
    from vent_analysis_amd import Vent_Analysis
    shape = (64, 64, 24)
    hp, mk = D.batch_inputs(shape), D.batch_masks(shape)
    for search, patch, rician in ((3, 1, False), (5, 2, True)):
        got = _lib.denoise(hp, D.SIGMAS, D.STRENGTH, search, patch, rician)
        assert same_bits(got, D.batch_reference(shape, search, patch, rician))
    one = _lib.denoise(hp[1], D.SIGMAS[1])            # a 3-D volume, a scalar sigma
    assert same_bits(one[0], D.batch_reference(shape, 3, 1, False)[1])
    est = _lib.noise_sigma(hp, mk)
    va = Vent_Analysis(pickle_dict=dict(HPvent=hp[0].copy(), mask=mk[0].astype(np.float64), vox=list(D.VOX)))
    before = {k: (v.copy() if isinstance(v, (np.ndarray, dict)) else v) for k, v in vars(va).items()}
    s = va.estimate_noise()
    out = va.denoise()
    fixed = va.denoise(sigma=D.SIGMAS[0], search=5, patch=2, rician=True)
    other = va.denoise(hp[1], sigma=D.SIGMAS[1])
    assert set(vars(va)) == set(before)
    np.testing.assert_equal(dict(vars(va)), before)
    assert isinstance(s, F32) and s.tobytes() == est[0].tobytes()
    assert same_bits(out, D.denoise(hp[0], s))
    assert same_bits(fixed, D.batch_reference(shape, 5, 2, True)[0])
    assert same_bits(other, D.batch_reference(shape, 3, 1, False)[1])
