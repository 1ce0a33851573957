"""Gaussian smoothing without a GPU: vr_smooth_weights (the one place the weights are computed), what the C ABI refuses, and
known answers of the CPU definition (tests/smooth_ref/smooth_ref.c), which tests/test_smoothing_gpu.py holds the kernels to."""
import ctypes as C
import importlib.util
import math
from pathlib import Path

import numpy as np
import pytest

_spec = importlib.util.spec_from_file_location("smooth_ref_binding", Path(__file__).resolve().parent / "smooth_ref" / "binding.py")
smooth_ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(smooth_ref)

SIGMAS = (0.3, 0.5, 1.0, 2.5, 8.0)


@pytest.fixture(scope="module")
def smoothlib(tmp_path_factory):
    return smooth_ref.build(tmp_path_factory.mktemp("smooth_ref"))


def weights_for(vra, sigmas):
    return tuple(vra.smooth_weights(s) if s > 0 else None for s in sigmas)


def test_library_exports_the_smoothing_entry_points(vra):
    lib = C.CDLL(str(vra.LIB_PATH))
    for name in ("vr_smooth_volume", "vr_get_smoothing", "vr_smooth_weights", "vr_set_smoothing_workspace", "vr_get_smoothing_ms"):
        assert hasattr(lib, name)
        assert name in vra.symbols_declared_in_header()


@pytest.mark.parametrize("sigma", SIGMAS)
def test_weights_radius_symmetry_accuracy_and_sum(vra, sigma):
    w = vra.smooth_weights(sigma)
    s = float(np.float32(sigma))                         # the value the C ABI receives
    r = math.ceil(3.0 * s)
    assert w.dtype == np.float32 and w.size == 2 * r + 1
    assert np.array_equal(w.view(np.uint32), w[::-1].view(np.uint32))          # symmetric bit for bit
    t = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-t * t / (2.0 * s * s))
    want = g / g.sum()
    ulp = np.spacing(want.astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(w.astype(np.float64) - want) <= ulp)                  # within 1 fp32 ulp of the float64 evaluation
    assert abs(float(w.astype(np.float64).sum()) - 1.0) <= 2.0 ** -20


def test_weights_are_refused_for_bad_sigmas_and_short_buffers(vra):
    lib = vra.load_library()
    R = vra.renderer
    buf = np.full(49, -1.0, dtype=np.float32)
    fp = buf.ctypes.data_as(C.POINTER(C.c_float))
    r = C.c_int(-7)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 8.0001, 9.0):
        assert lib.vr_smooth_weights(bad, fp, 49, C.byref(r)) == R.VR_E_INVALID
    assert lib.vr_smooth_weights(1.0, fp, 6, C.byref(r)) == R.VR_E_INVALID    # needs 2 * 3 + 1
    assert lib.vr_smooth_weights(8.0, fp, 48, C.byref(r)) == R.VR_E_INVALID   # needs 49
    assert lib.vr_smooth_weights(1.0, None, 49, C.byref(r)) == R.VR_E_INVALID
    assert r.value == -7 and np.all(buf == -1.0)                              # a refused call writes nothing
    assert lib.vr_smooth_weights(1.0, fp, 7, None) == R.VR_OK                 # exactly enough; the radius is optional
    assert lib.vr_smooth_weights(8.0, fp, 49, C.byref(r)) == R.VR_OK and r.value == 24
    with pytest.raises(vra.VRError):
        vra.smooth_weights(0.0)


def test_host_only_handle_refuses_smoothing(vra):
    R = vra.renderer
    r = vra.RendererCore(-1)
    r.setup((64, 64))
    assert r.smoothing == (0.0, 0.0, 0.0)
    with pytest.raises(vra.VRError) as e:
        r.smoothVolume(sigma_voxels=(1.0, 1.0, 1.0))
    assert e.value.code == R.VR_E_NO_DEVICE
    for bad in ((-0.5, 1, 1), (1, float("nan"), 1), (1, 1, 8.5), (float("inf"), 0, 0)):
        with pytest.raises(vra.VRError) as e:
            r.smoothVolume(sigma_voxels=bad)
        assert e.value.code == R.VR_E_INVALID                                  # the arguments are checked first
    assert r.smoothing == (0.0, 0.0, 0.0)
    with pytest.raises(ValueError):
        r.smoothVolume()
    with pytest.raises(ValueError):
        r.smoothVolume(sigma_voxels=1.0, sigma_mm=1.0)
    r.close()


@pytest.mark.parametrize("dtype,value", [(np.uint8, 0), (np.uint8, 255), (np.uint8, 77), (np.uint16, 65535), (np.uint16, 4095), (np.uint16, 1)])
def test_a_constant_volume_is_unchanged(vra, smoothlib, dtype, value):
    vol = np.full((6, 11, 13), value, dtype=dtype)
    for sig in ((0.3, 0.3, 0.3), (1.0, 2.5, 0.5), (8.0, 8.0, 8.0), (0.0, 0.0, 2.5)):
        got = smooth_ref.smooth(smoothlib, vol, weights_for(vra, sig))
        assert np.array_equal(got, vol), sig


def test_a_pass_along_x_leaves_a_volume_that_varies_along_y_or_z_alone(vra, smoothlib):
    rng = np.random.default_rng(5)
    for dtype, hi in ((np.uint8, 256), (np.uint16, 65536)):
        prof_y = rng.integers(0, hi, size=11).astype(dtype)
        prof_z = rng.integers(0, hi, size=6).astype(dtype)
        vy = np.broadcast_to(prof_y[None, :, None], (6, 11, 13)).copy()
        vz = np.broadcast_to(prof_z[:, None, None], (6, 11, 13)).copy()
        for s in SIGMAS:
            w = weights_for(vra, (s, 0.0, 0.0))
            assert np.array_equal(smooth_ref.smooth(smoothlib, vy, w), vy)
            assert np.array_equal(smooth_ref.smooth(smoothlib, vz, w), vz)


def test_no_pass_at_all_is_the_identity(vra, smoothlib):
    vol = np.random.default_rng(6).integers(0, 65536, size=(6, 11, 13)).astype(np.uint16)
    assert np.array_equal(smooth_ref.smooth(smoothlib, vol, (None, None, None)), vol)


def test_a_single_bright_voxel_becomes_the_outer_product_of_the_weights(vra, smoothlib):
    sig = (1.0, 0.5, 2.5)
    wx, wy, wz = weights_for(vra, sig)
    rx, ry, rz = [(w.size - 1) // 2 for w in (wx, wy, wz)]
    for dtype, peak in ((np.uint8, 255), (np.uint16, 65535)):
        vol = np.zeros((2 * rz + 3, 2 * ry + 3, 2 * rx + 3), dtype=dtype)
        c = (rz + 1, ry + 1, rx + 1)
        vol[c] = peak
        got = smooth_ref.smooth(smoothlib, vol, (wx, wy, wz))
        # x: w_x * peak (one product, added to 0); y: w_y * that; z: w_z * that -- fp32 products in this order, then the rounding
        fx = (wx * np.float32(peak)).astype(np.float32)
        fxy = (wy[:, None] * fx[None, :]).astype(np.float32)
        fxyz = (wz[:, None, None] * fxy[None, :, :]).astype(np.float32)
        want = np.zeros_like(vol)
        want[1:-1, 1:-1, 1:-1] = np.clip(np.rint(fxyz), 0, peak).astype(dtype)
        assert np.array_equal(got, want)
        assert got[c] == np.rint(fxyz[rz, ry, rx]) and got.sum() > 0


@pytest.mark.parametrize("sigma", (0.5, 1.0, 2.5))
def test_permuting_axes_and_sigmas_together_permutes_the_output(vra, smoothlib, sigma):
    vol = np.random.default_rng(7).integers(0, 65536, size=(6, 11, 13)).astype(np.uint16)     # [z, y, x]
    w = vra.smooth_weights(sigma)
    along_x = smooth_ref.smooth(smoothlib, vol, (w, None, None))
    # the same data with x and y (x and z) exchanged, smoothed along the axis the data's x went to
    xy = np.ascontiguousarray(vol.transpose(0, 2, 1))
    assert np.array_equal(smooth_ref.smooth(smoothlib, xy, (None, w, None)).transpose(0, 2, 1), along_x)
    xz = np.ascontiguousarray(vol.transpose(2, 1, 0))
    assert np.array_equal(smooth_ref.smooth(smoothlib, xz, (None, None, w)).transpose(2, 1, 0), along_x)


@pytest.mark.parametrize("sig", [(1.0, 1.0, 1.0), (0.5, 2.0, 0.0), (0.0, 0.0, 3.0), (8.0, 0.3, 1.0), (0.0, 1.0, 0.0)])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_the_pointwise_entry_point_agrees_with_the_whole_volume_one(vra, smoothlib, sig, dtype):
    hi = 256 if dtype == np.uint8 else 65536
    vol = np.random.default_rng(8).integers(0, hi, size=(6, 11, 13)).astype(dtype)
    w = weights_for(vra, sig)
    whole = smooth_ref.smooth(smoothlib, vol, w)
    kk, jj, ii = np.meshgrid(np.arange(6), np.arange(11), np.arange(13), indexing="ij")
    ijk = np.stack([ii.ravel(), jj.ravel(), kk.ravel()], axis=1)
    pts = smooth_ref.smooth_points(smoothlib, vol, w, ijk)
    assert np.array_equal(pts.reshape(6, 11, 13), whole)


def test_smoothing_reduces_noise_and_keeps_the_mean(vra, smoothlib):
    """a sanity anchor against a float64 numpy evaluation of the same separable sum (loose: the definition's roundings differ)"""
    vol = np.random.default_rng(9).integers(1000, 3000, size=(9, 12, 14)).astype(np.uint16)
    sig = (1.0, 2.0, 0.5)
    w = weights_for(vra, sig)
    got = smooth_ref.smooth(smoothlib, vol, w).astype(np.float64)
    ref = vol.astype(np.float64)
    for axis, wa in zip((2, 1, 0), w):
        r = (wa.size - 1) // 2
        idx = np.clip(np.arange(ref.shape[axis])[:, None] + np.arange(-r, r + 1)[None, :], 0, ref.shape[axis] - 1)
        ref = np.moveaxis((np.take(ref, idx, axis=axis) * wa.astype(np.float64).reshape((1,) * axis + (1, -1) + (1,) * (2 - axis))).sum(axis=axis + 1), axis, axis)
    assert np.max(np.abs(got - ref)) <= 0.5 + 3000 * 3 * 49 * 2.0 ** -23
    assert got.std() < vol.std()
