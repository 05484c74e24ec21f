"""CPU: the host side of the proton resampler -- vh_resample_taps (no device) against the numpy reference
bit for bit, grid_map, the binding's argument checks, and the reference (resample_ref) against itself."""
import ctypes as ct

import numpy as np
import pytest

from vent_analysis_amd import _lib

import resample_ref as F


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_symbols_are_exported_and_signed():
    L = _lib.lib()
    for name in ("vh_resample_taps", "vh_batch_upload_proton_src", "vh_batch_resample_proton",
                 "vh_batch_download_proton_src", "vh_resample"):
        assert hasattr(L, name) and name in _lib._SIGS, name
    assert L.vh_abi_version() == 8
    assert _lib.RESAMPLE_TAPS == F.TAPS == 8
    for name in ("upload_proton_src", "resample_proton", "download_proton_src"):
        assert callable(getattr(_lib.Batch, name))


@pytest.mark.parametrize("n_src,n_dst", [(83, 41), (21, 41), (1, 12), (5, 9)], ids=str)
def test_taps_equal_the_reference_bit_for_bit(n_src, n_dst):
    most = 0
    for scale in F.SCALES:
        for offset in F.offsets(n_src):
            got = _lib.resample_taps(n_src, n_dst, scale, offset)
            want = F.taps(n_src, n_dst, scale, offset)
            assert got[0].dtype == got[1].dtype == np.int32 and got[2].dtype == np.float32
            assert got[2].shape == (n_dst, 8)
            for g, w, what in zip(got, want, ("first", "count", "weight")):
                assert same(g, w), (scale, offset, what)
            assert got[1].min() >= 0 and got[1].max() <= 8                  # never more than 8 taps
            most = max(most, int(got[1].max()))
            if offset == n_src + 6.0:                                       # wholly outside
                assert not got[1].any() and not got[0].any() and not got[2].any()
    assert most == (8 if n_src >= 8 else n_src)                             # ... and 8 are reached


def test_the_known_tables():
    first, count, weight = _lib.resample_taps(9, 9, 1.0, 0.0)
    assert first.tolist() == list(range(9)) and count.tolist() == [1] * 9
    assert same(weight[:, 0], np.ones(9, np.float32)) and not weight[:, 1:].any()
    first, count, weight = _lib.resample_taps(16, 8, 2.0, 0.5)
    assert first[1:7].tolist() == [1, 3, 5, 7, 9, 11] and count.tolist() == [3, 4, 4, 4, 4, 4, 4, 3]
    assert same(weight[1:7, :4], np.tile(np.array([0.125, 0.375, 0.375, 0.125], np.float32), (6, 1)))
    assert same(weight[0, :3], np.array([0.375, 0.375, 0.125], np.float32)) and not weight[:, 4:].any()
    assert _lib.resample_taps(5, 4, 1.0, 11.0)[1].tolist() == [0] * 4
    L = _lib.lib()
    f, c, w = np.zeros(4, np.int32), np.zeros(4, np.int32), np.zeros((4, 8), np.float32)
    p = _lib._ptr
    assert L.vh_resample_taps(4, 4, 1.0, 0.0, p(f), p(c), p(w)) == _lib.VH_OK
    for bad in ((0, 4, 1.0, 0.0), (1025, 4, 1.0, 0.0), (4, 0, 1.0, 0.0), (4, 4, 0.2, 0.0), (4, 4, 4.5, 0.0),
                (4, 4, float("nan"), 0.0), (4, 4, 1.0, float("inf")), (4, 4, 1.0, 2.0 ** 20 + 1)):
        assert L.vh_resample_taps(*bad, p(f), p(c), p(w)) == _lib.VH_ERR_ARG, bad
        with pytest.raises(ValueError):
            _lib.resample_taps(*bad)
    assert L.vh_resample_taps(4, 4, 1.0, 0.0, None, p(c), p(w)) == _lib.VH_ERR_ARG
    assert L.vh_resample_taps(4, 4, 1.0, 0.0, p(f), None, p(w)) == _lib.VH_ERR_ARG
    assert L.vh_resample_taps(4, 4, 1.0, 0.0, p(f), p(c), None) == _lib.VH_ERR_ARG


def test_grid_map_against_hand_values():
    m = _lib.grid_map((256, 256, 24), (0.75, 0.75, 10.0), (128, 128, 24), (1.5, 1.5, 10.0))
    assert m.dtype == np.float64 and m.shape == (3, 2) and m.flags.c_contiguous
    assert m.tolist() == [[2.0, 0.5], [2.0, 0.5], [1.0, 0.0]]           # 127.5 - 2 * 63.5
    m = _lib.grid_map((256, 256, 24), (0.75, 0.75, 10.0), (128, 128, 24), (1.5, 1.5, 10.0), shift=(3, -2, 1))
    assert m.tolist() == [[2.0, 6.5], [2.0, -3.5], [1.0, 1.0]]          # + scale * shift
    m = _lib.grid_map((83, 75, 9), (1.0, 1.0, 8.0), (41, 37, 5), (2.0, 2.0, 16.0))
    assert m.tolist() == [[2.0, 1.0], [2.0, 1.0], [2.0, 0.0]]           # 41 - 40, 37 - 36, 4 - 4
    m = _lib.grid_map((21, 19, 5), (3.0, 3.0, 20.0), (41, 37, 9), (1.5, 1.5, 10.0), shift=(0.5, 0, 0))
    assert m.tolist() == [[0.5, 0.25], [0.5, 0.0], [0.5, 0.0]]          # a larger, coarser source: upsampling
    for bad in (((256, 256), (1, 1, 1), (128, 128, 24), (1, 1, 1)), ((256, 256, 0), (1, 1, 1), (128, 128, 24), (1, 1, 1)),
                ((4, 4, 4), (1, 1, 0), (4, 4, 4), (1, 1, 1)), ((4, 4, 4), (1, 1, 1), (4, 4, 4), (1, -1, 1)),
                ((4, 4, 4), (1, 1), (4, 4, 4), (1, 1, 1)), ((4.0, 4.0, 4.0), (1, 1, 1), (4, 4, 4), (1, 1, 1)),
                ((4, 4, 4), (1, 1, float("nan")), (4, 4, 4), (1, 1, 1)), ((4, 4, 4), "abc", (4, 4, 4), (1, 1, 1))):
        with pytest.raises(ValueError):
            _lib.grid_map(*bad)
    with pytest.raises(ValueError):
        _lib.grid_map((4, 4, 4), (1, 1, 1), (4, 4, 4), (1, 1, 1), shift=(1, 2))


def test_argument_checks_run_before_any_device_call():
    one = [[2.0, 0.5], [2.0, 0.5], [1.0, 0.0]]
    m = _lib._resample_args(one, 3, (256, 256, 24))
    assert m.dtype == np.float64 and m.shape == (3, 3, 2) and m.flags.c_contiguous and m[2].tolist() == one
    assert _lib._resample_args([one, one], 2).shape == (2, 3, 2)
    assert _lib._resample_args([[1, 0], [1, 0], [1, 0]], 1).dtype == np.float64          # ints are numbers
    assert _lib._resample_args([[0.25, -2.0 ** 20], [4.0, 2.0 ** 20], [1.0, 0.0]], 1).shape == (1, 3, 2)
    nan, inf = float("nan"), float("inf")
    for bad in ([[0.2, 0.0], [1.0, 0.0], [1.0, 0.0]], [[1.0, 0.0], [4.01, 0.0], [1.0, 0.0]],
                [[1.0, 0.0], [1.0, 0.0], [nan, 0.0]], [[1.0, nan], [1.0, 0.0], [1.0, 0.0]],
                [[1.0, 0.0], [1.0, inf], [1.0, 0.0]], [[1.0, 0.0], [1.0, 0.0], [1.0, -2.0 ** 20 - 1]],
                [[-1.0, 0.0], [1.0, 0.0], [1.0, 0.0]], [[inf, 0.0], [1.0, 0.0], [1.0, 0.0]],
                [[1.0, 0.0], [1.0, 0.0]], [one] * 2, [1.0, 0.0], None, "map", [[True, False]] * 3):
        with pytest.raises(ValueError):
            _lib._resample_args(bad, 3)
    for shape in ((0, 4, 4), (4, 1025, 4), (4, 4), (4.0, 4.0, 4.0)):
        with pytest.raises(ValueError):
            _lib._resample_args(one, 1, shape)
    # the module-level call refuses before it touches a context
    x = np.ones((8, 8, 2), np.float32)
    for args in ((x, (4, 4, 2), [[9.0, 0.0], [1.0, 0.0], [1.0, 0.0]]), (x, (4, 4), one), (x, (1, 4, 2), one),
                 (np.ones((8, 8), np.float32), (4, 4, 2), one), (np.ones((2, 1025, 2), np.float32), (4, 4, 2), one),
                 (x, (4, 4, 2), [one, one])):
        with pytest.raises(ValueError):
            _lib.resample(*args, device=10 ** 6)
    # ... and so does the class method
    from vent_analysis_amd import Vent_Analysis
    shape = (41, 37, 9)
    va = Vent_Analysis(pickle_dict=dict(HPvent=np.ones(shape, np.float32), mask=np.ones(shape), vox=[1.5, 1.5, 10.0]))
    va.device = 10 ** 6
    with pytest.raises(ValueError):
        va.resample_proton(proton_vox=(0.75, 0.75, 10.0))                  # no proton
    va.proton = np.ones((83, 75))
    with pytest.raises(ValueError):
        va.resample_proton(proton_vox=(0.75, 0.75, 10.0))                  # not 3-D
    va.proton = np.ones((83, 75, 9))
    with pytest.raises(ValueError):
        va.resample_proton()                                               # no header to read the voxel size from
    with pytest.raises(ValueError):
        va.resample_proton(proton_vox=(0.1, 0.75, 10.0))                   # scale 15
    with pytest.raises(ValueError):
        va.resample_proton(proton_vox=(0.75, 0.75))
    with pytest.raises(ValueError):
        va.resample_proton(proton_vox=(0.75, 0.75, 10.0), shift=(2.0 ** 20, 0, 0))
    va.proton = np.ones((1025, 75, 9))
    with pytest.raises(ValueError):
        va.resample_proton(proton_vox=(0.75, 0.75, 10.0))                  # a source dimension beyond 1024
    L = _lib.lib()
    assert L.vh_batch_upload_proton_src(None, None, None) == _lib.VH_ERR_ARG
    assert L.vh_batch_resample_proton(None, None) == _lib.VH_ERR_ARG
    assert L.vh_batch_download_proton_src(None, None) == _lib.VH_ERR_ARG
    assert L.vh_resample(None, None, None, 4, 4, 2, 1, None, None) == _lib.VH_ERR_ARG


def test_the_reference_itself():
    """The vectorised passes equal the per-voxel nested loop byte for byte; the identity returns the source;
    scale 1 with integer offsets is the zero-filled shift."""
    import register_ref as G
    src_shape, dst_shape = (9, 8, 5), (6, 11, 4)
    m = [(1.7, -0.4), (0.6, 0.3), (1.3, 0.2)]
    S = F.study(src_shape, 3)
    assert same(F.resample(S, dst_shape, m), F.resample_nested(S, dst_shape, m))
    S = S.copy()
    S[4, 3, 2] = np.nan
    S[0, 0, 0] = -0.0
    a, b = F.resample(S, dst_shape, m), F.resample_nested(S, dst_shape, m)
    assert same(np.isnan(a), np.isnan(b)) and np.isnan(a).any() and not np.isnan(a).all()
    assert same(np.nan_to_num(a, nan=-1.0), np.nan_to_num(b, nan=-1.0))
    ident = [(1.0, 0.0)] * 3
    out = F.resample(S, src_shape, ident)
    assert np.array_equal(out, S, equal_nan=True) and not np.signbit(out[0, 0, 0])    # -0.0 becomes +0.0
    for s in ((2, -3, 1), (-9, 0, 0), (0, 7, -4)):
        got = F.resample(S, src_shape, [(1.0, float(d)) for d in s])
        assert np.array_equal(got, G.shift_image(S, s), equal_nan=True)
    Sb, M = F.batch((21, 19, 5), (41, 37, 9))
    assert Sb.shape == (4, 21, 19, 5) and M.shape == (4, 3, 2) and not Sb.flags.writeable
    assert same(F.reference((21, 19, 5), (41, 37, 9))[2], F.resample(Sb[2], (41, 37, 9), M[2]))
