"""Gradient-lit compositing without a GPU: the C ABI's entry points and their host-side checks, and known answers of the
mode's CPU definition (tests/shade_ref/shade_ref.c) -- at (1, 0, 0) it is the composite mode (the oracle's frames and counts,
the executed reference's goldens), for any coefficients its alpha plane and counts are the composite mode's, a ramp along the
view axis lights its centre ray by the closed form, and zero-alpha entries of the transfer function add nothing."""
import ctypes as C
import importlib.util
import json
import math
from pathlib import Path

import numpy as np
import pytest

_spec = importlib.util.spec_from_file_location("shade_ref_binding", Path(__file__).resolve().parent / "shade_ref" / "binding.py")
shade_ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(shade_ref)

GOLD = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="session")
def shadelib(tmp_path_factory):
    return shade_ref.build(tmp_path_factory.mktemp("shade_ref"))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def orbit_cam(oracle, zenith=0.0, azimuth=0.0, zoom_in=0):
    c = oracle.Camera()
    for _ in range(zoom_in):
        c.orient(1.0, 0.0, 0.0)
    if zenith or azimuth:
        c.orient(0.0, zenith, azimuth)
    return c.block()


def test_library_exports_the_shading_entry_points(vra):
    lib = C.CDLL(str(vra.LIB_PATH))
    for name in ("vr_set_shading", "vr_get_shading"):
        assert hasattr(lib, name)
        assert name in vra.symbols_declared_in_header()


def test_host_only_handle_checks_arguments_and_round_trips(vra):
    R = vra.renderer
    r = vra.RendererCore(-1)
    r.setup((64, 64))
    assert r.loadShader("VolumeRenderer.cs")
    st = r.shading()
    assert st["enable"] is False and st["shininess"] == 16
    assert (st["ambient"], st["diffuse"], st["specular"]) == tuple(float(np.float32(v)) for v in (0.15, 0.65, 0.2))
    r.setShading(True, 0.25, 0.5, 0.125, 64)
    want = dict(enable=True, ambient=0.25, diffuse=0.5, specular=0.125, shininess=64)
    assert r.shading() == want
    for shin in (1, 2, 4, 8, 16, 32, 64, 128):
        r.setShading(True, 0.25, 0.5, 0.125, shin)
        assert r.shading()["shininess"] == shin
    r.setShading(True, 0.25, 0.5, 0.125, 64)
    bad = [(-0.1, 0.5, 0.1, 16), (0.1, -1e-30, 0.1, 16), (0.1, 0.5, -2.0, 16), (math.nan, 0.5, 0.1, 16), (0.1, math.inf, 0.1, 16),
           (0.1, 0.5, -math.inf, 16), (0.1, 0.5, 0.1, 0), (0.1, 0.5, 0.1, 3), (0.1, 0.5, 0.1, 256), (0.1, 0.5, 0.1, -16), (0.1, 0.5, 0.1, 48)]
    for args in bad:
        with pytest.raises(vra.VRError) as e:
            r.setShading(True, *args)
        assert e.value.code == R.VR_E_INVALID, args
        assert r.shading() == want, args                 # a refused call changes nothing
    # enable = 0 ignores the other arguments, always succeeds and keeps the coefficients
    r.setShading(False, math.nan, -1.0, math.inf, 3)
    assert r.shading() == dict(want, enable=False)
    # zeros are valid coefficients
    r.setShading(True, 0.0, 0.0, 0.0, 1)
    assert r.shading() == dict(enable=True, ambient=0.0, diffuse=0.0, specular=0.0, shininess=1)
    # neither the isosurface nor the reslice mode refuses it, nor does it refuse them; the state is kept
    r.setIsosurface(True, 100)
    r.setShading(True, 1.0, 0.0, 0.0, 8)
    r.setIsosurface(False, 100)
    r.setReslice(True, np.zeros(12, dtype=np.float32), mode="mip", n=1)
    r.setShading(True, 1.0, 0.0, 0.0, 8)
    r.setReslice(False)
    assert r.shading() == dict(enable=True, ambient=1.0, diffuse=0.0, specular=0.0, shininess=8)
    for call in (lambda: r.render(), lambda: r.renderAsync(), lambda: r.countSamples()):
        with pytest.raises(vra.VRError) as e:
            call()
        assert e.value.code == R.VR_E_NO_DEVICE
    r.close()


def test_null_handle_is_refused(vra):
    lib = vra.load_library()
    R = vra.renderer
    assert lib.vr_set_shading(None, 1, 0.1, 0.2, 0.3, 16) == R.VR_E_INVALID
    assert lib.vr_set_shading(None, 0, 0.1, 0.2, 0.3, 16) == R.VR_E_INVALID
    assert lib.vr_get_shading(None, None, None, None, None, None) == R.VR_E_INVALID


TF_ISO = [0, 60, 140, 255]
TF_RGBA = [[0.2, 0.9, 0.1, 0.0], [0.9, 0.3, 0.2, 0.4], [1.0, 0.8, 0.6, 0.8], [0.5, 0.5, 1.0, 1.0]]


def _lut(vra):
    r = vra.RendererCore(-1)
    r.setTransferFunction(TF_ISO, TF_RGBA)
    lut = r.getTransferLut()
    r.close()
    return lut


_POSES = [dict(), dict(zenith=0.6, azimuth=0.9), dict(zenith=-0.4, azimuth=2.5), dict(zoom_in=3), dict(zoom_in=2, zenith=0.3, azimuth=-0.4)]   # zoom_in=3: the eye at the box centre


def _cases(vra, oracle, n, seed):
    """a seeded matrix of small composite configurations (u8 / u16, both filters and accumulation modes, three views, TF or
    not, odd dims, anisotropic spacing, poses with the eye inside the box)"""
    rng = np.random.default_rng(seed)
    lut = _lut(vra)
    for case in range(n):
        dtype = np.uint8 if case % 2 == 0 else np.uint16
        dims = tuple(int(v) for v in rng.integers(9, 40, size=3))
        if case % 3 == 0:
            dims = (dims[0] | 1, dims[1] | 1, dims[2])
        spacing = (1.0, 1.0, 1.0) if case % 4 == 0 else tuple(float(v) for v in rng.uniform(0.5, 2.0, size=3).round(2))
        vol = oracle.gen_noise_ball(dims, np.dtype(dtype).itemsize, int(rng.integers(1 << 31)))
        view = ["front", "top", "bottom"][case % 3]
        lo, hi = (int(rng.integers(0, 40)), int(rng.integers(120, 256))) if dtype == np.uint8 else (int(rng.integers(0, 1500)), int(rng.integers(2000, 4096)))
        yield case, vol, dict(cam=orbit_cam(oracle, **_POSES[case % len(_POSES)]), voxel_size=spacing, min_val=lo, max_val=hi,
                              view_top=int(view == "top"), view_bottom=int(view == "bottom"), filter=(case // 2) % 2,
                              accum=(case // 4) % 2, alpha_scale=float(rng.choice([0.02, 0.3, 1.0])),
                              tf_rgba=lut if (case // 3) % 2 == 1 else None)


def test_unit_ambient_is_the_composite_mode_bit_for_bit(vra, oracle, shadelib):
    n_lit = 0
    for case, vol, kw in _cases(vra, oracle, 24, 31):
        p = oracle.OracleParams(37, 29, **kw)
        want, _, want_spp = oracle.render(vol, p, want_spp=True)
        for shin in (1, 16, 128):
            got, spp = shade_ref.render(shadelib, vol, p, 1.0, 0.0, 0.0, shin)
            assert np.array_equal(bits(got), bits(want)), f"case {case} shininess {shin}"
            assert np.array_equal(spp, want_spp), f"case {case}"
        n_lit += int((want[..., 3] > 0).sum())
    assert n_lit > 1000


def test_any_coefficients_keep_the_composite_alpha_and_counts(vra, oracle, shadelib):
    for case, vol, kw in _cases(vra, oracle, 16, 32):
        p = oracle.OracleParams(33, 27, **kw)
        want, _, want_spp = oracle.render(vol, p, want_spp=True)
        for coef in ((0.15, 0.65, 0.2, 16), (0.0, 1.0, 0.0, 1), (0.3, 2.5, 0.7, 128)):
            got, spp = shade_ref.render(shadelib, vol, p, *coef)
            assert np.array_equal(bits(got[..., 3]), bits(want[..., 3])), f"case {case} {coef}"
            assert np.array_equal(spp, want_spp), f"case {case} {coef}"
            if kw["tf_rgba"] is None:
                assert np.array_equal(bits(got[..., 0]), bits(got[..., 1])) and np.array_equal(bits(got[..., 0]), bits(got[..., 2]))
        # and the lighting does change the colour somewhere
        lit, _ = shade_ref.render(shadelib, vol, p)
        assert not np.array_equal(bits(lit[..., :3]), bits(want[..., :3])) or (want[..., 3] == 0).all()


_MANIFEST = json.loads((GOLD / "ref_gl_manifest.json").read_text())
_GOLD_CASES = sorted(n for n, c in _MANIFEST["cases"].items() if not c["mip"] and np.prod(c["vol"][1]) <= 2 ** 28)


@pytest.mark.parametrize("name", _GOLD_CASES)
def test_unit_ambient_matches_the_executed_reference_goldens(oracle, shadelib, name):
    c = _MANIFEST["cases"][name]
    spec = c["vol"]
    vol = oracle.gen_sphere_u8(spec[1], spec[2]) if spec[0] == "sphere" else oracle.gen_noise_ball(tuple(spec[1]), spec[2], spec[3])
    z = np.load(GOLD / "ref_gl" / f"{name}.npz")
    rows, ga = z["rows"], z["ga"]
    W, H = c["img"]
    lo, hi = c["uploaded_window"]
    cam = np.frombuffer(bytes.fromhex("".join(c["cam_f32_hex"])), dtype=np.float32).copy()
    p = oracle.OracleParams(W, H, cam=cam, alpha_scale=c["alpha"], voxel_size=tuple(c["spacing"]), min_val=lo, max_val=hi,
                            view_top=c["top"], view_bottom=c["bottom"], trunc_grid=1,
                            filter=1 if c.get("filter") == "trilinear" else 0, row_begin=int(rows.min()), row_end=int(rows.max()) + 1)
    got, _ = shade_ref.render(shadelib, vol, p, 1.0, 0.0, 0.0, 16)
    g = got[rows]
    want = np.stack([ga[..., 0], ga[..., 0], ga[..., 0], ga[..., 1]], axis=-1)
    assert np.array_equal(bits(g), bits(want)), f"{name}: {int((bits(g) != bits(want)).any(axis=-1).sum())} pixels differ"


@pytest.mark.parametrize("view", ["front", "top", "bottom"])
@pytest.mark.parametrize("filt", [0, 1])
@pytest.mark.parametrize("coef", [(0.15, 0.65, 0.2, 16), (0.3, 0.9, 0.5, 1), (0.05, 0.4, 0.0, 128)])
def test_ramp_along_the_view_axis_lights_the_centre_ray_by_the_closed_form(oracle, shadelib, view, filt, coef):
    # the ramp runs along the volume axis behind box z (front: z, top / bottom: y); the centre pixel of an odd frame looks
    # straight down box z, so N = +-z, d = 1 and every sample's colour is min(c * (ambient + diffuse) + specular, 1)
    n = 32
    k, j, i = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    ramp = ((k if view == "front" else j) * 4 + 60).astype(np.uint8)
    c_rgb = np.array([0.3, 0.55, 0.8], dtype=np.float32)
    tf = np.zeros((256, 4), dtype=np.float32)
    tf[:, :3] = c_rgb
    tf[:, 3] = 0.35
    amb, dif, spec, shin = coef
    f32 = np.float32
    k_rgb = np.minimum(c_rgb * (f32(amb) + f32(dif)) + f32(spec), f32(1.0)).astype(np.float32)   # d = 1: d^shininess = 1
    kw = dict(view_top=int(view == "top"), view_bottom=int(view == "bottom"), filter=filt, alpha_scale=0.5, min_val=0, max_val=255)
    W = H = 33
    got, spp = shade_ref.render(shadelib, ramp, oracle.OracleParams(W, H, tf_rgba=tf, **kw), *coef)
    tf_k = tf.copy()
    tf_k[:, :3] = k_rgb
    want, _, want_spp = oracle.render(ramp, oracle.OracleParams(W, H, tf_rgba=tf_k, **kw), want_spp=True)
    c = (H // 2, W // 2)
    assert spp[c] > 10 and spp[c] == want_spp[c]
    if filt == 0:
        # NEAREST differences are whole multiples of the ramp step, the scales powers of two: N and d are exact
        assert np.array_equal(bits(got[c]), bits(want[c])), (got[c], want[c])
    else:
        # TRILINEAR: |G| is not a power of two, N may land an ulp off the axis length, d^shininess a few ulps below 1
        np.testing.assert_allclose(got[c], want[c], rtol=0, atol=2e-5)
        assert bits(got[c][3]) == bits(want[c][3])


@pytest.mark.parametrize("filt", [0, 1])
def test_zero_alpha_entries_add_nothing_whatever_their_colour(vra, oracle, shadelib, filt):
    vol = oracle.gen_noise_ball((31, 28, 26), 1, 17)
    lut = _lut(vra)
    dirty = lut.reshape(256, 4).copy()
    zero = dirty[:, 3] == 0.0
    assert zero.sum() >= 1
    clean = dirty.copy()
    clean[zero, :3] = 0.0
    dirty[zero, :3] = np.array([1.0, 0.25, 0.75], dtype=np.float32)
    kw = dict(cam=orbit_cam(oracle, 0.3, 0.4), filter=filt, alpha_scale=0.4, min_val=0, max_val=200)
    a, sa = shade_ref.render(shadelib, vol, oracle.OracleParams(41, 35, tf_rgba=dirty, **kw), 0.2, 0.7, 0.4, 8)
    b, sb = shade_ref.render(shadelib, vol, oracle.OracleParams(41, 35, tf_rgba=clean, **kw), 0.2, 0.7, 0.4, 8)
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(sa, sb)
    assert (a[..., 3] > 0).sum() > 100
