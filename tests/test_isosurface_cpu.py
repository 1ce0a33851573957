"""The first-hit isosurface mode without a GPU: the C ABI's entry points, their host-side checks, and known answers of its
CPU definition (tests/iso_ref/iso_ref.c) -- normals of linear ramps, the sphere's depth, and the march geometry it shares
with the composite mode (its sample counts when nothing is hit are the oracle's at alpha_scale 0)."""
import ctypes as C
import importlib.util
import itertools
from pathlib import Path

import numpy as np
import pytest

_spec = importlib.util.spec_from_file_location("iso_ref_binding", Path(__file__).resolve().parent / "iso_ref" / "binding.py")
iso_ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(iso_ref)


@pytest.fixture(scope="session")
def isolib(tmp_path_factory):
    return iso_ref.build(tmp_path_factory.mktemp("iso_ref"))


def test_library_exports_the_isosurface_entry_points(vra):
    lib = C.CDLL(str(vra.LIB_PATH))
    assert hasattr(lib, "vr_set_isosurface") and hasattr(lib, "vr_read_depth")
    assert "vr_set_isosurface" in vra.symbols_declared_in_header() and "vr_read_depth" in vra.symbols_declared_in_header()


def test_host_only_handle_sets_the_mode_and_fails_loudly_on_gpu_work(vra):
    r = vra.RendererCore(-1)
    r.setup((64, 64))
    assert r.loadShader("VolumeRenderer.cs")
    r.setIsosurface(True, 300)
    r.setIsosurface(False, 300)
    r.setIsosurface(True, -1000)
    for call in (lambda: r.render(), lambda: r.renderAsync(), lambda: r.countSamples(), lambda: r.readDepth()):
        with pytest.raises(vra.VRError) as e:
            call()
        assert e.value.code == vra.renderer.VR_E_NO_DEVICE
    r.close()


def test_read_depth_argument_checks(vra):
    lib = vra.load_library()
    assert lib.vr_read_depth(None, None, 0) == vra.renderer.VR_E_INVALID
    assert lib.vr_set_isosurface(None, 1, 0) == vra.renderer.VR_E_INVALID


def test_greyalpha_target_refuses_isosurface_frames(vra):
    r = vra.RendererCore(-1)
    r.setup((64, 64))
    assert r.loadShader("VolumeRenderer.cs")
    r.setFramebufferExternal(0x1000)        # never dereferenced: the frame is refused before any device work
    r.setFramebufferFormat(vra.renderer.FB_GREYALPHA32F)
    r.setIsosurface(True, 100)
    for call in (lambda: r.render(), lambda: r.renderAsync(), lambda: r.countSamples()):
        with pytest.raises(vra.VRError) as e:
            call()
        assert e.value.code == vra.renderer.VR_E_INVALID
    # the same target without the mode is a device error on this handle, not a format error
    r.setIsosurface(False, 100)
    with pytest.raises(vra.VRError) as e:
        r.render()
    assert e.value.code == vra.renderer.VR_E_NO_DEVICE
    r.close()


def _orbit_cam(oracle, zenith=0.0, azimuth=0.0, zoom_in=0):
    c = oracle.Camera()
    for _ in range(zoom_in):
        c.orient(1.0, 0.0, 0.0)
    if zenith or azimuth:
        c.orient(0.0, zenith, azimuth)
    return c.block()


# box axis behind each volume axis, per view (vr_core.h: vr_set_isosurface, step 4)
_BOX_AXIS = {"front": (0, 1, 2), "top": (0, 2, 1), "bottom": (0, 2, 1)}


@pytest.mark.parametrize("view", ["front", "top", "bottom"])
@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("filt", [0, 1])
@pytest.mark.parametrize("dims,spacing", [((32, 32, 32), (1.0, 1.0, 1.0)), ((64, 32, 16), (1.0, 2.0, 0.5)), ((16, 32, 64), (2.0, 1.0, 1.0))])
def test_linear_ramp_normal_is_exactly_the_box_axis(oracle, isolib, view, axis, filt, dims, spacing):
    nx, ny, nz = dims
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    ramp = (i, j, k)[axis].astype(np.uint16) * 16 + 100
    n_axis = dims[axis]
    iso = 100 + 16 * (n_axis // 2) + 5 - 1000          # between two voxel values, mid-volume (u16: the +1000 offset)
    p = oracle.OracleParams(48, 40, cam=_orbit_cam(oracle, 0.35, 0.5), voxel_size=spacing, min_val=0, max_val=4095,
                            view_top=int(view == "top"), view_bottom=int(view == "bottom"), filter=filt)
    rgba, depth, spp, nrm = iso_ref.render(isolib, ramp, p, iso, want_normal=True)
    hit = np.isfinite(depth)
    assert hit.sum() > 50, "the pose must show the iso plane"
    box = _BOX_AXIS[view][axis]
    n = nrm[hit]
    # NEAREST differences are whole multiples of the ramp's step and the scales are powers of two: |G| is one, N exact.  The
    # TRILINEAR lerps round, so |G| is not a power of two and N = v * (1 / sqrt(dot)) may land one ulp below 1 (never above)
    lo = np.float32(1.0) if filt == 0 else np.nextafter(np.float32(1.0), np.float32(0.0))
    assert np.all((np.abs(n[:, box]) >= lo) & (np.abs(n[:, box]) <= 1.0)), n[np.abs(n[:, box]) < lo][:4]
    others = [a for a in range(3) if a != box]
    assert np.all(n[:, others] == 0.0)
    assert np.all(rgba[hit][:, 3] == 1.0) and np.all(rgba[~hit] == 0.0)
    assert np.all(spp[hit] >= 1)


@pytest.mark.parametrize("filt", [0, 1])
def test_sphere_centre_pixel_faces_the_eye_at_eye_distance_minus_radius(oracle, isolib, filt):
    vol = oracle.gen_sphere_u8(64, 28)
    # v = 255 - (255 * isqrt(r2)) // 56 >= 128  <=>  isqrt(r2) <= 28: the surface at 14 voxels = 14 / 64 box units
    p = oracle.OracleParams(64, 64, filter=filt)
    rgba, depth, spp, nrm = iso_ref.render(isolib, vol, p, 128, want_normal=True)
    c = (32, 32)
    step = 1.0 / 64.0                                  # length(1, 1, 1) / length(64, 64, 64)
    assert abs(float(depth[c]) - (3.0 - 14.0 / 64.0)) <= step
    assert nrm[c][2] > 0.999 and rgba[c][3] == 1.0
    assert rgba[c][0] > 0.95                           # head-on: 0.15 + 0.65 + 0.2, nearly white
    # no surface behind the camera's view of the box corners: misses are the reference's background
    assert np.all(rgba[~np.isfinite(depth)] == 0.0)


def test_transfer_function_sets_the_base_colour(oracle, isolib):
    vol = oracle.gen_sphere_u8(32, 14)
    tf = np.zeros((256, 4), dtype=np.float32)
    tf[:, 0] = 1.0; tf[:, 1] = np.linspace(0, 1, 256); tf[:, 3] = 1.0
    p = oracle.OracleParams(32, 32, tf_rgba=tf, min_val=0, max_val=255)
    rgba, depth, _ = iso_ref.render(isolib, vol, p, 100)
    hit = np.isfinite(depth)
    assert hit.any()
    idx = int(np.floor(np.float32(100.0 / 255.0) * np.float32(255.0) + np.float32(0.5)))
    assert np.all(rgba[hit][:, 2] <= 0.2 + 1e-6)      # blue base 0: only the highlight
    assert np.all(rgba[hit][:, 0] >= rgba[hit][:, 1])
    assert 0 < idx < 255


_POSES = [dict(), dict(zenith=0.6, azimuth=0.9), dict(zenith=-0.4, azimuth=2.5), dict(zoom_in=3), dict(zoom_in=3, zenith=0.3, azimuth=0.2)]


@pytest.mark.parametrize("pose", range(len(_POSES)))
@pytest.mark.parametrize("view,spacing,dtype", [("front", (1.0, 1.0, 1.0), np.uint8), ("top", (0.7, 1.3, 1.0), np.uint16),
                                                ("bottom", (1.0, 0.5, 2.0), np.uint8), ("front", (1.5, 1.0, 0.8), np.uint16)])
@pytest.mark.parametrize("accum", [0, 1])
def test_no_hit_counts_are_the_composite_geometry(oracle, isolib, pose, view, spacing, dtype, accum):
    vol = oracle.gen_noise_ball((37, 30, 26), np.dtype(dtype).itemsize, 11)
    vmax = int(vol.max())
    off = 1000 if dtype == np.uint16 else 0
    cam = _orbit_cam(oracle, **_POSES[pose])
    kw = dict(cam=cam, voxel_size=spacing, view_top=int(view == "top"), view_bottom=int(view == "bottom"), accum=accum,
              min_val=0, max_val=vmax)
    for filt in (0, 1):
        p = oracle.OracleParams(45, 33, filter=filt, **kw)
        rgba, depth, spp = iso_ref.render(isolib, vol, p, vmax + 1 - off)
        _, _, want = oracle.render(vol, oracle.OracleParams(45, 33, filter=filt, alpha_scale=0.0, **kw), want_spp=True)
        assert np.array_equal(spp, want)
        assert np.all(rgba == 0.0) and np.all(np.isinf(depth))
        assert want.sum() > 0


def test_iso_below_the_minimum_hits_at_the_first_sample(oracle, isolib):
    vol = oracle.gen_noise_ball((24, 24, 24), 1, 3)
    p = oracle.OracleParams(40, 40, cam=_orbit_cam(oracle, 0.4, 0.3))
    rgba, depth, spp = iso_ref.render(isolib, vol, p, 0)
    _, _, marched = oracle.render(vol, oracle.OracleParams(40, 40, cam=p.cam, alpha_scale=0.0), want_spp=True)
    inside = marched > 0
    assert np.all(spp[inside] == 1) and np.all(spp[~inside] == 0)
    assert np.all(np.isfinite(depth[inside])) and np.all(rgba[inside][:, 3] == 1.0)


def test_row_range_renders_only_its_rows(oracle, isolib):
    vol = oracle.gen_sphere_u8(32, 14)
    full = iso_ref.render(isolib, vol, oracle.OracleParams(40, 36), 90)
    part = iso_ref.render(isolib, vol, oracle.OracleParams(40, 36, row_begin=10, row_end=23), 90)
    for a, b in zip(full, part):
        assert np.array_equal(a[10:23], b[10:23])
    assert np.all(part[2][:10] == 0) and np.all(np.isinf(part[1][23:]))
