"""The multi-planar reslice mode without a GPU: the C ABI's entry points and their host-side checks, known answers of its CPU
definition (tests/reslice_ref/reslice_ref.c) against numpy -- windowed slices, slab maxima / minima / means, the inside test,
counts, the HU read-back and the transfer function -- and the geometry helpers of renderer.py."""
import ctypes as C
import importlib.util
from pathlib import Path

import numpy as np
import pytest

_spec = importlib.util.spec_from_file_location("reslice_ref_binding", Path(__file__).resolve().parent / "reslice_ref" / "binding.py")
reslice_ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(reslice_ref)

QNAN = 0x7FC00000


@pytest.fixture(scope="session")
def rslib(tmp_path_factory):
    return reslice_ref.build(tmp_path_factory.mktemp("reslice_ref"))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def f32(*v):
    return np.array(v, dtype=np.float32)


def axial(k, dz=1.0):
    """pixel (x, y) -> voxel (x, y, k), slab steps dz along z"""
    return np.concatenate([f32(0, 0, k), f32(1, 0, 0), f32(0, 1, 0), f32(0, 0, dz)])


def window(v, lo, hi):
    """the composite mode's window on float32 values (max == min: 0)"""
    v = np.asarray(v, dtype=np.float32)
    lo32, hi32 = np.float32(lo), np.float32(hi)
    if hi == lo:
        return np.zeros_like(v)
    c = np.minimum(np.maximum(v, lo32), hi32)
    return ((c - lo32) / np.float32(hi - lo)).astype(np.float32)


def vol_u8(shape=(20, 17, 23), seed=1):
    return np.random.default_rng(seed).integers(0, 256, size=shape).astype(np.uint8)


# ---------------------------------------------------------------- the C ABI


def test_library_exports_the_reslice_entry_points(vra):
    lib = C.CDLL(str(vra.LIB_PATH))
    assert hasattr(lib, "vr_set_reslice") and hasattr(lib, "vr_read_reslice_values")
    declared = vra.symbols_declared_in_header()
    assert "vr_set_reslice" in declared and "vr_read_reslice_values" in declared
    R = vra.renderer
    assert (R.VR_SLAB_MIP, R.VR_SLAB_MINIP, R.VR_SLAB_MEAN) == (0, 1, 2)


def test_host_only_handle_sets_and_clears_the_mode(vra):
    R = vra.renderer
    r = vra.RendererCore(-1)
    r.setup((64, 64))
    assert r.loadShader("VolumeRenderer.cs")
    g = axial(3.0)
    r.setReslice(True, g[:3], g[3:6], g[6:9], g[9:], mode="mip", n=7)
    r.setReslice(True, g, mode="mean", n=1024)
    r.setReslice(True, g, mode=R.VR_SLAB_MINIP, n=1)
    r.setReslice(False)
    r.setReslice(False)
    r.setReslice(True, g)
    for call in (lambda: r.render(), lambda: r.renderAsync(), lambda: r.countSamples()):
        with pytest.raises(vra.VRError) as e:
            call()
        assert e.value.code == R.VR_E_NO_DEVICE
    r.close()


def test_invalid_arguments_are_refused(vra):
    R = vra.renderer
    lib = vra.load_library()
    assert lib.vr_set_reslice(None, 0, None, 0, 1) == R.VR_E_INVALID
    assert lib.vr_read_reslice_values(None, None, 0) == R.VR_E_INVALID
    r = vra.RendererCore(-1)
    r.setup((32, 32))
    g = np.ascontiguousarray(axial(1.0))
    fp = g.ctypes.data_as(C.POINTER(C.c_float))
    for mode, n in ((3, 1), (-1, 1), (0, 0), (1, 1025), (2, -4)):
        assert lib.vr_set_reslice(r._h, 1, fp, mode, n) == R.VR_E_INVALID, (mode, n)
    assert lib.vr_set_reslice(r._h, 1, None, 0, 1) == R.VR_E_INVALID
    for bad in (np.nan, np.inf, -np.inf):
        for i in (0, 4, 8, 11):
            h = g.copy()
            h[i] = bad
            assert lib.vr_set_reslice(r._h, 1, h.ctypes.data_as(C.POINTER(C.c_float)), 0, 1) == R.VR_E_INVALID, (bad, i)
    # enable = 0 ignores everything else
    assert lib.vr_set_reslice(r._h, 0, None, 7, 0) == R.VR_OK
    assert lib.vr_set_reslice(r._h, 1, fp, 2, 1024) == R.VR_OK
    r.close()


def test_isosurface_and_reslice_exclude_each_other(vra):
    R = vra.renderer
    r = vra.RendererCore(-1)
    r.setup((32, 32))
    g = axial(0.0)
    r.setIsosurface(True, 100)
    with pytest.raises(vra.VRError) as e:
        r.setReslice(True, g)
    assert e.value.code == R.VR_E_INVALID
    r.setReslice(False)                     # switching off always succeeds
    r.setIsosurface(False, 100)
    r.setReslice(True, g)
    with pytest.raises(vra.VRError) as e:
        r.setIsosurface(True, 100)
    assert e.value.code == R.VR_E_INVALID
    r.setIsosurface(False, 0)
    r.setReslice(False)
    r.setIsosurface(True, 100)
    r.close()


def test_read_values_before_any_reslice_frame_is_invalid(vra):
    r = vra.RendererCore(-1)
    r.setup((16, 16))
    with pytest.raises(vra.VRError) as e:
        r.readResliceValues()
    assert e.value.code == vra.renderer.VR_E_INVALID
    r.setReslice(True, axial(0.0))
    with pytest.raises(vra.VRError) as e:
        r.readResliceValues()
    assert e.value.code == vra.renderer.VR_E_INVALID
    r.close()


# ---------------------------------------------------------------- known answers of the definition


@pytest.mark.parametrize("lo,hi", [(0, 255), (30, 200), (77, 77)])
def test_axis_aligned_nearest_slice_is_the_numpy_windowed_slice(rslib, lo, hi):
    vol = vol_u8()
    nz, ny, nx = vol.shape
    for k in (0, 7, nz - 1):
        rgba, values, cnt = reslice_ref.render(rslib, vol, axial(k), nx, ny, min_val=lo, max_val=hi)
        v = window(vol[k].astype(np.float32), lo, hi)
        assert np.array_equal(bits(rgba[..., 0]), bits(v)) and np.array_equal(bits(rgba[..., 2]), bits(v))
        assert np.all(rgba[..., 3] == 1.0)
        assert np.array_equal(bits(values), bits(vol[k].astype(np.float32)))
        assert np.all(cnt == 1)


@pytest.mark.parametrize("m", [1, 3])
def test_mip_and_minip_slabs_along_z_are_numpy_max_and_min(rslib, m):
    vol = vol_u8(seed=2)
    nz, ny, nx = vol.shape
    k = 8
    for mode, ref in (("mip", vol[k - m:k + m + 1].max(0)), ("minip", vol[k - m:k + m + 1].min(0))):
        rgba, values, cnt = reslice_ref.render(rslib, vol, axial(k), nx, ny, mode=mode, n=2 * m + 1)
        assert np.array_equal(bits(values), bits(ref.astype(np.float32))), mode
        assert np.all(cnt == 2 * m + 1)
        assert np.array_equal(bits(rgba[..., 1]), bits(window(ref, 0, 255)))


def test_mean_is_a_sequential_float32_sum_over_the_count(rslib):
    vol = np.random.default_rng(3).integers(0, 4096, size=(30, 9, 11)).astype(np.uint16)
    nz, ny, nx = vol.shape
    for k, n in ((12, 7), (14, 64), (1, 6)):          # (the last two reach outside the volume: fewer samples count)
        rgba, values, cnt = reslice_ref.render(rslib, vol, axial(k), nx, ny, mode="mean", n=n, u16_offset=False)
        acc = np.zeros((ny, nx), dtype=np.float32)
        c = 0
        for j in range(n):
            z = k + (2 * j - (n - 1)) * 0.5
            r = z + 0.5
            if 0 <= r < nz:
                acc = (acc + vol[int(r)].astype(np.float32)).astype(np.float32)
                c += 1
        assert np.all(cnt == c)
        assert np.array_equal(bits(values), bits(acc / np.float32(c)))


def test_a_plane_partly_outside_is_background_exactly_where_r_leaves_the_volume(rslib):
    vol = vol_u8(shape=(12, 14, 16), seed=4)
    nz, ny, nx = vol.shape
    w, h = 40, 31
    g = np.concatenate([f32(-7.3, -5.6, 3.2), f32(0.61, 0.13, 0.07), f32(-0.09, 0.58, 0.21), f32(0, 0, 1)])
    for filt in (0, 1):
        rgba, values, cnt = reslice_ref.render(rslib, vol, g, w, h, filt=filt)
        X = np.arange(w, dtype=np.float32)[None, :]
        Y = np.arange(h, dtype=np.float32)[:, None]
        inside = np.ones((h, w), dtype=bool)
        for a, dim in enumerate((nx, ny, nz)):
            p = ((g[a] + X * g[3 + a]).astype(np.float32) + Y * g[6 + a]).astype(np.float32)
            r = (p + np.float32(0.5)).astype(np.float32)
            inside &= (r >= 0) & (r < np.float32(dim))
        assert 0 < inside.sum() < inside.size
        assert np.array_equal(cnt == 1, inside) and np.all(cnt[~inside] == 0)
        assert np.all(rgba[~inside] == 0.0) and np.all(bits(values[~inside]) == QNAN)
        assert np.all(rgba[inside][:, 3] == 1.0) and not np.isnan(values[inside]).any()


def test_trilinear_at_integer_positions_equals_nearest(rslib):
    vol = vol_u8(seed=5)
    nz, ny, nx = vol.shape
    # integer positions, not axis-aligned: du steps one voxel in x and y, dv one in y and z
    g = np.concatenate([f32(0, 0, 2), f32(1, 1, 0), f32(0, 1, 1), f32(1, 0, 1)])
    for mode, n in (("mip", 1), ("minip", 3), ("mean", 5)):
        a = reslice_ref.render(rslib, vol, g, 30, 20, mode=mode, n=n, filt=0)
        b = reslice_ref.render(rslib, vol, g, 30, 20, mode=mode, n=n, filt=1)
        for x, y in zip(a, b):
            assert np.array_equal(bits(x), bits(y)) if x.dtype == np.float32 else np.array_equal(x, y)
        assert (a[2] > 0).sum() > 100


def test_the_three_modes_agree_at_n_1(rslib):
    vol = np.random.default_rng(6).integers(0, 4096, size=(13, 15, 17)).astype(np.uint16)
    g = np.concatenate([f32(-2.2, 1.3, 4.7), f32(0.37, 0.21, -0.11), f32(0.05, 0.44, 0.29), f32(0.3, -0.2, 0.9)])
    for filt in (0, 1):
        out = [reslice_ref.render(rslib, vol, g, 33, 27, mode=m, n=1, filt=filt, min_val=900, max_val=4200) for m in ("mip", "minip", "mean")]
        for o in out[1:]:
            assert np.array_equal(bits(o[0]), bits(out[0][0])) and np.array_equal(bits(o[1]), bits(out[0][1]))
            assert np.array_equal(o[2], out[0][2])


def test_counts_are_the_inside_samples(rslib):
    vol = vol_u8(shape=(10, 8, 9), seed=7)
    nz, ny, nx = vol.shape
    for k, n, dz in ((0, 7, 1.0), (9, 7, 1.0), (4, 64, 0.25), (5, 2, 3.0)):
        _, _, cnt = reslice_ref.render(rslib, vol, axial(k, dz), nx, ny, mode="mean", n=n)
        want = sum(1 for j in range(n) if 0 <= np.float32(k) + np.float32((2 * j - (n - 1)) * 0.5) * np.float32(dz) + np.float32(0.5) < nz)
        assert np.all(cnt == want), (k, n, dz)


def test_u16_values_are_read_back_in_hounsfield_units_under_the_offset(rslib):
    vol = np.random.default_rng(8).integers(0, 3000, size=(6, 7, 8)).astype(np.uint16)
    nz, ny, nx = vol.shape
    _, hu, _ = reslice_ref.render(rslib, vol, axial(2), nx, ny, min_val=0, max_val=4000, u16_offset=True)
    _, raw, _ = reslice_ref.render(rslib, vol, axial(2), nx, ny, min_val=0, max_val=4000, u16_offset=False)
    assert np.array_equal(bits(raw), bits(vol[2].astype(np.float32)))
    assert np.array_equal(bits(hu), bits(vol[2].astype(np.float32) - np.float32(1000.0)))
    # 8-bit data ignore the offset
    v8 = vol_u8(shape=(6, 7, 8))
    _, val8, _ = reslice_ref.render(rslib, v8, axial(2), nx, ny, u16_offset=True)
    assert np.array_equal(bits(val8), bits(v8[2].astype(np.float32)))


def test_transfer_function_sets_the_colour(rslib):
    vol = vol_u8(seed=9)
    nz, ny, nx = vol.shape
    tf = np.zeros((256, 4), dtype=np.float32)
    tf[:, 0] = np.linspace(0, 1, 256)
    tf[:, 1] = np.linspace(1, 0, 256)
    tf[:, 2] = 0.25
    tf[:, 3] = 0.5                                   # alpha of the entry is not used: reslice pixels are opaque
    lo, hi = 20, 220
    rgba, _, _ = reslice_ref.render(rslib, vol, axial(5), nx, ny, min_val=lo, max_val=hi, tf_rgba=tf)
    v = window(vol[5], lo, hi)
    idx = np.clip(np.floor((v * np.float32(255.0)).astype(np.float32) + np.float32(0.5)), 0, 255).astype(np.int64)
    assert np.array_equal(bits(rgba[..., :3]), bits(tf[idx][..., :3]))
    assert np.all(rgba[..., 3] == 1.0)


# ---------------------------------------------------------------- geometry helpers


def test_axis_planes_give_the_exact_vectors(vra, rslib):
    dims = (23, 17, 20)
    # anisotropic spacing: the axial pixels are the in-plane voxels, the slab step one voxel along z
    g = vra.axis_reslice("axial", 7, dims, (0.5, 0.5, 2.0), (23, 17))
    assert np.array_equal(g, np.concatenate([f32(0, 0, 7), f32(1, 0, 0), f32(0, 1, 0), f32(0, 0, 1)])), g
    for sp in ((1.0, 1.0, 1.0), (2.0, 2.0, 2.0)):
        g = vra.axis_reslice("axial", 7, dims, sp, (23, 17))
        assert np.array_equal(g, np.concatenate([f32(0, 0, 7), f32(1, 0, 0), f32(0, 1, 0), f32(0, 0, 1)])), g
        g = vra.axis_reslice("coronal", 5, dims, sp, (23, 20))
        assert np.array_equal(g, np.concatenate([f32(0, 5, 0), f32(1, 0, 0), f32(0, 0, 1), f32(0, -1, 0)])), g
        g = vra.axis_reslice("sagittal", 11, dims, sp, (17, 20))
        assert np.array_equal(g, np.concatenate([f32(11, 0, 0), f32(0, 1, 0), f32(0, 0, 1), f32(1, 0, 0)])), g
    assert np.array_equal(vra.axis_reslice(2, 3, dims, (1, 1, 1), (23, 17)), vra.axis_reslice("axial", 3, dims, (1, 1, 1), (23, 17)))
    # through the definition: the axial helper renders the slice itself
    vol = vol_u8()
    nz, ny, nx = vol.shape
    _, values, _ = reslice_ref.render(rslib, vol, vra.axis_reslice("axial", 9, (nx, ny, nz), (1, 1, 1), (nx, ny)), nx, ny)
    assert np.array_equal(values, vol[9].astype(np.float32))
    with pytest.raises(ValueError):
        vra.axis_reslice("axial", 0, dims, (1, 1, 1), (8, 8), n=0)


def test_axis_planes_fit_the_volume_with_square_pixels(vra):
    dims, sp = (100, 60, 40), (0.5, 1.0, 2.0)
    g = vra.axis_reslice("coronal", 30, dims, sp, (64, 64))
    du_mm, dv_mm = g[3:6] * np.asarray(sp), g[6:9] * np.asarray(sp)
    assert np.isclose(np.linalg.norm(du_mm), np.linalg.norm(dv_mm))
    pix = np.linalg.norm(du_mm)
    assert np.isclose(pix, max(50.0 / 64, 80.0 / 64))          # x: 50 mm, z: 80 mm across


def test_oblique_frames_are_orthonormal_in_mm(vra):
    rng = np.random.default_rng(10)
    for _ in range(50):
        sp = rng.uniform(0.3, 2.5, size=3)
        normal, up = rng.normal(size=3), rng.normal(size=3)
        pix, step = rng.uniform(0.2, 3.0), rng.uniform(0.2, 3.0)
        g = vra.reslice_geometry((64, 50, 40), sp, rng.uniform(0, 50, size=3), normal, up, pix, step, (97, 61)).astype(np.float64)
        eu, ev, ew = g[3:6] * sp / pix, g[6:9] * sp / pix, g[9:12] * sp / step
        for a in (eu, ev, ew):
            assert abs(np.linalg.norm(a) - 1.0) < 1e-6
        assert abs(eu @ ev) < 1e-6 and abs(eu @ ew) < 1e-6 and abs(ev @ ew) < 1e-6
        assert np.allclose(ew, normal / np.linalg.norm(normal), atol=1e-6)
        assert np.linalg.det(np.stack([eu, ev, ew])) > 0                  # columns, rows, normal: right-handed
        assert ev @ up > 0                                               # rows advance along `up`


def test_the_plane_centre_maps_to_the_image_centre(vra):
    rng = np.random.default_rng(11)
    for w, h in ((64, 64), (97, 61), (1920, 1080)):
        sp = rng.uniform(0.3, 2.5, size=3)
        c = rng.uniform(0, 80, size=3)
        g = vra.reslice_geometry((128, 128, 128), sp, c, rng.normal(size=3), rng.normal(size=3), 0.7, 1.0, (w, h)).astype(np.float64)
        centre = g[0:3] + ((w - 1) / 2.0) * g[3:6] + ((h - 1) / 2.0) * g[6:9]
        assert np.allclose(centre, c / sp, rtol=0, atol=1e-4 * max(1.0, np.abs(c / sp).max()))
