"""The gradient-lit composite kernel (vr_shade.hip) against its CPU definition (tests/shade_ref/shade_ref.c): RGBA bits and
per-pixel sample counts over a seeded matrix of small frames, the cfg3 and 2048^3 shapes on sampled rows, skipping on and off,
row shards, stripes, compact and (grey, alpha) targets, a three-member group; and its place among the modes -- at (1, 0, 0) it
is the composite kernels' frame, MIP frames ignore it, the isosurface and reslice modes take precedence, and a round trip
leaves the composite frames and the measured launch choices untouched."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("shade_ref_binding", Path(__file__).resolve().parent / "shade_ref" / "binding.py")
shade_ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(shade_ref)

KERNEL = "raymarch_shade_kernel"


@pytest.fixture(scope="session")
def shadelib(tmp_path_factory):
    return shade_ref.build(tmp_path_factory.mktemp("shade_ref_gpu"))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(got, want, what):
    for name, g, w in zip(("rgba", "spp"), got, want):
        ok = np.array_equal(g, w) if name == "spp" else np.array_equal(bits(g), bits(w))
        if not ok:
            bad = np.argwhere(g != w) if name == "spp" else np.argwhere(bits(g) != bits(w))
            y, x = bad[0][:2]
            raise AssertionError(f"{what}: {name} differs at {len(bad)} places, first (row {y}, col {x}): {g[y, x]} vs {w[y, x]}")


def orbit_cam(oracle, zenith=0.0, azimuth=0.0, zoom_in=0):
    c = oracle.Camera()
    for _ in range(zoom_in):
        c.orient(1.0, 0.0, 0.0)
    if zenith or azimuth:
        c.orient(0.0, zenith, azimuth)
    return c.block()


def hip_frame(r):
    r.render()
    rgba = r.readPixels()
    _, spp = r.countSamples(per_pixel=True)
    return rgba, spp


TF_ISO = [0, 60, 140, 255]
TF_RGBA = [[0.2, 0.9, 0.1, 0.0], [0.9, 0.3, 0.2, 0.4], [1.0, 0.8, 0.6, 0.8], [0.5, 0.5, 1.0, 1.0]]
COEFS = [(0.15, 0.65, 0.2, 16), (1.0, 0.0, 0.0, 16), (0.3, 1.7, 0.6, 1), (0.0, 0.9, 0.35, 128), (0.05, 0.4, 0.9, 2)]


def test_random_matrix_matches_the_reference(vra, oracle, shadelib):
    rng = np.random.default_rng(20261017)
    poses = [dict(), dict(zenith=0.5, azimuth=0.8), dict(zenith=-0.7, azimuth=2.2), dict(zoom_in=3), dict(zoom_in=2, zenith=0.3, azimuth=-0.4),
             dict(zenith=1.2, azimuth=0.1)]
    r = vra.RendererCore(0)
    try:
        for case in range(120):
            dtype = np.uint8 if rng.integers(2) == 0 else np.uint16
            dims = tuple(int(v) for v in rng.integers(9, 48, size=3))
            if case % 5 == 0:
                dims = (dims[0] | 1, dims[1], dims[2])          # nx % 4 != 0
            spacing = (1.0, 1.0, 1.0) if rng.integers(3) == 0 else tuple(float(v) for v in rng.uniform(0.5, 2.0, size=3).round(2))
            w, h = int(rng.integers(17, 70)), int(rng.integers(17, 70))
            vol = oracle.gen_noise_ball(dims, np.dtype(dtype).itemsize, int(rng.integers(1 << 31)))
            if rng.integers(3) == 0:
                vol = rng.integers(0, 256 if dtype == np.uint8 else 4096, size=vol.shape).astype(dtype)
            off = 1000 if dtype == np.uint16 else 0
            view = ["front", "top", "bottom"][int(rng.integers(3))]
            filt, layout, accum, skip = (int(v) for v in rng.integers(2, size=4))
            use_tf = rng.integers(2) == 1
            lo, hi = (int(rng.integers(0, 40)), int(rng.integers(120, 256))) if dtype == np.uint8 else (int(rng.integers(-1000, 500)), int(rng.integers(1500, 3100)))
            alpha = float(rng.choice([0.004, 0.05, 0.3, 1.0]))
            coef = COEFS[int(rng.integers(len(COEFS)))]
            cam = orbit_cam(oracle, **poses[int(rng.integers(len(poses)))])
            r.setup((w, h))
            assert r.loadShader("VolumeRenderer.cs")
            r.setLayout(layout)
            r.setVolume(vol, spacing)
            r.setInitialCameraRotation(view == "top", view == "bottom")
            r.setCameraBlock(cam)
            r.setFilter(filt)
            r.setAccum(accum)
            r.setWindow(lo, hi)
            r.setAlpha(alpha)
            r.setMIP(False)
            r.setSkipEmpty(bool(skip))
            r.setTransferFunction(TF_ISO, TF_RGBA) if use_tf else r.setTransferFunction()
            r.setShading(True, *coef)
            got = hip_frame(r)
            assert r.last_kernel_name == KERNEL and r.last_launch_choice == 0
            p = oracle.OracleParams(w, h, cam=cam, voxel_size=spacing, alpha_scale=alpha, min_val=lo + off, max_val=hi + off,
                                    view_top=int(view == "top"), view_bottom=int(view == "bottom"), filter=filt, accum=accum,
                                    tf_rgba=r.getTransferLut() if use_tf else None)
            want = shade_ref.render(shadelib, vol, p, *coef)
            assert_same(got, want, f"case {case}: {dtype.__name__} {dims} {spacing} {w}x{h} {view} filt {filt} layout {layout} "
                                   f"accum {accum} skip {skip} tf {use_tf} alpha {alpha} coef {coef}")
    finally:
        r.close()


def _sampled_rows_match(r, vol, shadelib, rows, coef, **kw):
    """the handle's last frame (rendered again for the counts) against the reference on `rows`"""
    w, h = r.framebuffer_size
    rgba = r.readPixels()
    _, spp = r.countSamples(per_pixel=True)
    for y in rows:
        want = shade_ref.render(shadelib, vol, __import__("oracle").OracleParams(w, h, row_begin=y, row_end=y + 1, **kw), *coef)
        assert_same((rgba[y:y + 1], spp[y:y + 1]), tuple(a[y:y + 1] for a in want), f"row {y}")


@pytest.fixture(scope="module")
def cfg3(vra):
    R = vra.renderer
    r = vra.RendererCore(0)
    r.setup((1920, 1080))
    assert r.loadShader("VolumeRenderer.cs")
    r.setLayout(R.LAYOUT_BRICKED)
    r.generateSynthetic(R.SYNTH_NOISE_BALL, (1024, 1024, 1024), 2, 0xC0FFEE)
    vol = r.readVolume()
    yield r, vol
    r.close()


@pytest.mark.parametrize("filt,skip,tf,pose", [(0, False, False, 0), (1, True, True, 1), (0, True, True, 1)])
def test_cfg3_sampled_rows_match_the_reference(vra, oracle, shadelib, cfg3, filt, skip, tf, pose):
    r, vol = cfg3
    cam = orbit_cam(oracle) if pose == 0 else orbit_cam(oracle, 0.5, 0.7)
    r.setCameraBlock(cam)
    r.setFilter(filt)
    r.setSkipEmpty(skip)
    r.setWindow(0, 3000)
    r.setAlpha(0.05)
    r.setTransferFunction(TF_ISO, TF_RGBA) if tf else r.setTransferFunction()
    r.setShading(True)
    r.render()
    assert r.last_kernel_name == KERNEL
    _sampled_rows_match(r, vol, shadelib, (0, 333, 540, 1079), COEFS[0], cam=cam, filter=filt, alpha_scale=0.05, min_val=1000,
                        max_val=4000, tf_rgba=r.getTransferLut() if tf else None)


def test_2048_cubed_u8_sampled_rows_match_the_reference(vra, oracle, shadelib):
    R = vra.renderer
    with vra.RendererCore(0) as r:
        r.setup((960, 540))
        assert r.loadShader("VolumeRenderer.cs")
        r.setLayout(R.LAYOUT_BRICKED)
        r.generateSynthetic(R.SYNTH_NOISE_BALL, (2048, 2048, 2048), 1, 0x9E3779B9)
        vol = r.readVolume()                   # 8 GiB over PCIe
        cam = orbit_cam(oracle, 0.3, 0.4)
        r.setCameraBlock(cam)
        r.setWindow(40, 255)
        r.setAlpha(0.02)
        r.setTransferFunction(TF_ISO, TF_RGBA)
        r.setSkipEmpty(True)
        r.setShading(True, *COEFS[2])
        for filt in (0, 1):
            r.setFilter(filt)
            r.render()
            assert r.last_kernel_name == KERNEL
            _sampled_rows_match(r, vol, shadelib, (100, 270, 431), COEFS[2], cam=cam, filter=filt, alpha_scale=0.02, min_val=40,
                                max_val=255, tf_rgba=r.getTransferLut())
        del vol


CFG2 = (512, 512, 452)


@pytest.fixture(scope="module")
def cfg2(vra):
    R = vra.renderer
    r = vra.RendererCore(0)
    r.setup((1920, 1080))
    assert r.loadShader("VolumeRenderer.cs")
    r.setLayout(R.LAYOUT_BRICKED)
    r.generateSynthetic(R.SYNTH_NOISE_BALL, CFG2, 2, 0x1234)
    yield r
    r.close()


@pytest.mark.parametrize("filt", [0, 1])
@pytest.mark.parametrize("tf,lo", [(False, 1200), (True, 0), (True, 1500)])
def test_skipping_is_invisible_at_the_cfg2_shape(vra, oracle, cfg2, filt, tf, lo):
    r = cfg2
    r.setFilter(filt)
    r.setCameraBlock(orbit_cam(oracle, 0.4, 0.6))
    r.setWindow(lo, 3000)
    r.setAlpha(0.1)
    r.setTransferFunction(TF_ISO, TF_RGBA) if tf else r.setTransferFunction()
    r.setShading(True)
    frames = {}
    for skip in (False, True):
        r.setSkipEmpty(skip)
        frames[skip] = hip_frame(r)
        assert r.last_kernel_name == KERNEL
    assert_same(frames[True], frames[False], f"skip on vs off, filter {filt}, tf {tf}, window from {lo}")
    assert (frames[True][0][..., 3] > 0).sum() > 1000


def _configure(r, vol, cam, filt, tf):
    r.setVolume(vol, (1.0, 1.2, 0.9))
    r.setCameraBlock(cam)
    r.setFilter(filt)
    r.setWindow(-200, 2500)
    r.setAlpha(0.08)
    r.setSkipEmpty(True)
    r.setTransferFunction(TF_ISO, TF_RGBA) if tf else r.setTransferFunction()
    r.setShading(True, 0.2, 0.7, 0.4, 8)


@pytest.mark.parametrize("filt,tf", [(0, False), (1, True), (1, False)])
def test_shards_stripes_and_targets_assemble_the_frame(vra, oracle, filt, tf):
    import torch

    R = vra.renderer
    sharding = __import__("importlib").import_module("volume-renderer_amd.sharding")
    vol = oracle.gen_noise_ball((61, 50, 47), 2, 5)
    cam = orbit_cam(oracle, 0.3, -0.5)
    size = (203, 157)
    w, h = size
    with vra.RendererCore(0) as r:
        r.setup(size)
        assert r.loadShader("VolumeRenderer.cs")
        _configure(r, vol, cam, filt, tf)
        full = hip_frame(r)
        assert r.last_kernel_name == KERNEL and (full[0][..., 3] > 0).sum() > 1000
        # contiguous shards on the own (full-size) target
        for b, e in ((0, 50), (50, 120), (120, 157)):
            r.setRowRange(b, e)
            part = hip_frame(r)
            assert_same(tuple(a[b:e] for a in part), tuple(a[b:e] for a in full), f"rows [{b}, {e})")
        r.setRowRange(0, -1)
        # cyclic stripes of 16 rows, three ways
        for idx in range(3):
            r.setRowStripes(16, idx, 3)
            part = hip_frame(r)
            rows = [y for y in range(h) if (y // 16) % 3 == idx]
            assert_same(tuple(a[rows] for a in part), tuple(a[rows] for a in full), f"stripe {idx}")
        r.setRowStripes(1, 0, 1)
        # compact external target, rendered asynchronously: rows 40..103 land at local rows 0..63
        tgt = torch.zeros((64, w, 4), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        r.setFramebufferExternal(tgt.data_ptr())
        r.setFramebufferCompact(True)
        r.setRowRange(40, 104)
        r.renderAsync()
        r.synchronize()
        assert r.last_kernel_name == KERNEL
        assert np.array_equal(bits(tgt.cpu().numpy()), bits(full[0][40:104]))
        r.setRowRange(0, -1)
        r.setFramebufferCompact(False)
        # (grey, alpha) target: grey modes only (no transfer function)
        ga = torch.full((h, w, 2), -1.0, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        r.setFramebufferExternal(ga.data_ptr())
        r.setFramebufferFormat(R.FB_GREYALPHA32F)
        if tf:
            with pytest.raises(vra.VRError) as e:
                r.render()
            assert e.value.code == R.VR_E_INVALID
        else:
            r.render()
            r.synchronize()
            assert np.array_equal(bits(sharding.expand_grey_alpha(ga).cpu().numpy()), bits(full[0]))
        r.setFramebufferExternal(0)
        r.setFramebufferFormat(R.FB_RGBA32F)
        del tgt, ga
    # a three-member group on device 0 (compact external targets; (grey, alpha) gather without a transfer function)
    with vra.RendererGroup([0, 0, 0]) as g:
        g.setup(size, partition="stripes", stripe_rows=16)

        def conf(m):
            m.loadShader("VolumeRenderer.cs")
            _configure(m, vol, cam, filt, tf)
        g.each(conf)
        g.render()
        got = g.readPixels()
    assert np.array_equal(bits(got), bits(full[0]))


@pytest.mark.parametrize("filt,tf,dtype,layout", [(0, False, np.uint16, 1), (0, True, np.uint8, 0), (1, False, np.uint8, 1), (1, True, np.uint16, 1)])
def test_unit_ambient_is_the_composite_kernels_frame(vra, oracle, filt, tf, dtype, layout):
    vol = oracle.gen_noise_ball((90, 77, 64), np.dtype(dtype).itemsize, 23)
    with vra.RendererCore(0) as r:
        r.setup((257, 199))
        assert r.loadShader("VolumeRenderer.cs")
        r.setLayout(layout)
        r.setVolume(vol, (1.0, 0.8, 1.1))
        r.setFilter(filt)
        r.setWindow(10, 220) if dtype == np.uint8 else r.setWindow(-300, 2800)
        r.setTransferFunction(TF_ISO, TF_RGBA) if tf else r.setTransferFunction()
        for k, (alpha, pose) in enumerate(((0.004, dict()), (0.3, dict(zenith=0.4, azimuth=0.7)), (1.0, dict(zoom_in=3)))):
            r.setCameraBlock(orbit_cam(oracle, **pose))
            r.setAlpha(alpha)
            r.setSkipEmpty(k == 1)
            r.setShading(False)
            plain = hip_frame(r)
            assert r.last_kernel_name != KERNEL
            r.setShading(True, 1.0, 0.0, 0.0, 32)
            lit = hip_frame(r)
            assert r.last_kernel_name == KERNEL
            assert_same(lit, plain, f"alpha {alpha} pose {pose}")
            r.setShading(True)
            shaded = hip_frame(r)
            assert np.array_equal(bits(shaded[0][..., 3]), bits(plain[0][..., 3])) and np.array_equal(shaded[1], plain[1])


def test_mip_frames_ignore_the_shading(vra, oracle):
    vol = oracle.gen_noise_ball((50, 41, 47), 2, 29)
    with vra.RendererCore(0) as r:
        r.setup((131, 97))
        assert r.loadShader("VolumeRenderer.cs")
        r.setVolume(vol)
        r.setCameraBlock(orbit_cam(oracle, 0.2, 0.5))
        r.setAlpha(0.6)
        r.setMIP(True)
        for filt in (0, 1):
            r.setFilter(filt)
            r.setShading(False)
            plain = hip_frame(r)
            r.setShading(True, 0.1, 0.9, 0.5, 4)
            got = hip_frame(r)
            assert r.last_kernel_name != KERNEL
            assert_same(got, plain, f"MIP, filter {filt}")
            assert r.shading()["enable"] is True


def test_composite_shaded_composite_leaves_the_composite_frames_and_choices(vra, oracle, shadelib):
    vol = oracle.gen_noise_ball((40, 36, 44), 1, 9)
    cam = orbit_cam(oracle, 0.2, 0.3)
    w, h = 97, 83
    with vra.RendererCore(0) as r:
        r.setup((w, h))
        assert r.loadShader("VolumeRenderer.cs")
        r.setVolume(vol)
        r.setCameraBlock(cam)
        r.setWindow(10, 200)
        r.setAlpha(0.3)
        r.setSkipEmpty(True)
        r.setAutotune(True)
        p = oracle.OracleParams(w, h, cam=cam, alpha_scale=0.3, min_val=10, max_val=200)
        want, _, want_spp = oracle.render(vol, p, want_spp=True)
        for _ in range(4):
            hip_frame(r)
        blobs = [r.exportChoices()]
        for step in range(3):
            r.setShading(step == 1, 0.1, 0.8, 0.3, 32)
            rgba, spp = hip_frame(r)
            if step == 1:
                assert r.last_kernel_name == KERNEL and r.last_launch_choice == 0
                assert_same((rgba, spp), shade_ref.render(shadelib, vol, p, 0.1, 0.8, 0.3, 32), "shaded")
                r.renderAsync()
                r.synchronize()
                blobs.append(r.exportChoices())
            else:
                assert r.last_kernel_name != KERNEL
                assert_same((rgba, spp), (want, want_spp), f"composite frame {step}")
        assert blobs[0] == blobs[1]


def test_isosurface_and_reslice_take_precedence_and_keep_the_shading(vra, oracle):
    vol = oracle.gen_noise_ball((40, 36, 44), 2, 13)
    w, h = 89, 71
    geom = vra.axis_reslice("axial", 20, (40, 36, 44), (1, 1, 1), (w, h), n=3)
    with vra.RendererCore(0) as r:
        r.setup((w, h))
        assert r.loadShader("VolumeRenderer.cs")
        r.setVolume(vol)
        r.setCameraBlock(orbit_cam(oracle, 0.3, 0.2))
        r.setAlpha(0.2)
        r.setIsosurface(True, 800)
        iso_plain = (hip_frame(r), r.readDepth())
        r.setShading(True, 0.3, 0.6, 0.1, 2)
        iso_shaded = (hip_frame(r), r.readDepth())
        assert r.last_kernel_name == "raymarch_iso_kernel"
        assert_same(iso_shaded[0], iso_plain[0], "isosurface")
        assert np.array_equal(bits(iso_shaded[1]), bits(iso_plain[1]))
        r.setIsosurface(False, 800)
        r.setShading(False)
        r.setReslice(True, geom, mode="mean", n=3)
        rs_plain = (hip_frame(r), r.readResliceValues())
        r.setShading(True, 0.3, 0.6, 0.1, 2)
        rs_shaded = (hip_frame(r), r.readResliceValues())
        assert r.last_kernel_name == "reslice_kernel"
        assert_same(rs_shaded[0], rs_plain[0], "reslice")
        assert np.array_equal(bits(rs_shaded[1]), bits(rs_plain[1]))
        r.setReslice(False)
        assert r.shading() == dict(enable=True, ambient=np.float32(0.3).item(), diffuse=np.float32(0.6).item(),
                                   specular=np.float32(0.1).item(), shininess=2)
        hip_frame(r)
        assert r.last_kernel_name == KERNEL
