"""The first-hit isosurface kernel (vr_iso.hip) against its CPU definition (tests/iso_ref/iso_ref.c): RGBA bits, depth bits
and per-pixel sample counts, over a seeded matrix of small frames, the cfg3 and 2048^3 shapes on sampled rows, row shards,
stripes, a three-member group, skipping on and off, and a mode round trip that must leave the composite frames untouched."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("iso_ref_binding", Path(__file__).resolve().parent / "iso_ref" / "binding.py")
iso_ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(iso_ref)


@pytest.fixture(scope="session")
def isolib(tmp_path_factory):
    return iso_ref.build(tmp_path_factory.mktemp("iso_ref_gpu"))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(got, want, what):
    for name, g, w in zip(("rgba", "depth", "spp"), got, want):
        if name == "spp":
            ok = np.array_equal(g, w)
        else:
            ok = np.array_equal(bits(g), bits(w))
        if not ok:
            bad = np.argwhere(bits(g) != bits(w)) if name != "spp" else np.argwhere(g != w)
            y, x = bad[0][:2]
            raise AssertionError(f"{what}: {name} differs at {len(bad)} places, first (row {y}, col {x}): {g[y, x]} vs {w[y, x]}")


def orbit_cam(oracle, zenith=0.0, azimuth=0.0, zoom_in=0):
    c = oracle.Camera()
    for _ in range(zoom_in):
        c.orient(1.0, 0.0, 0.0)
    if zenith or azimuth:
        c.orient(0.0, zenith, azimuth)
    return c.block()


def hip_iso(r, with_counts=True):
    r.render()
    rgba = r.readPixels()
    depth = r.readDepth()
    spp = r.countSamples(per_pixel=True)[1] if with_counts else None
    return rgba, depth, spp


TF_ISO = [0, 60, 140, 255]
TF_RGBA = [[0.2, 0.9, 0.1, 0.0], [0.9, 0.3, 0.2, 0.4], [1.0, 0.8, 0.6, 0.8], [0.5, 0.5, 1.0, 1.0]]


def test_random_matrix_matches_the_reference(vra, oracle, isolib):
    rng = np.random.default_rng(20261016)
    poses = [dict(), dict(zenith=0.5, azimuth=0.8), dict(zenith=-0.7, azimuth=2.2), dict(zoom_in=3), dict(zoom_in=2, zenith=0.3, azimuth=-0.4),
             dict(zenith=1.2, azimuth=0.1)]
    r = vra.RendererCore(0)
    try:
        n_frames = 0
        for case in range(150):
            dtype = np.uint8 if rng.integers(2) == 0 else np.uint16
            dims = tuple(int(v) for v in rng.integers(9, 48, size=3))
            if case % 5 == 0:
                dims = (dims[0] | 1, dims[1], dims[2])          # nx % 4 != 0
            spacing = (1.0, 1.0, 1.0) if rng.integers(3) == 0 else tuple(float(v) for v in rng.uniform(0.5, 2.0, size=3).round(2))
            w, h = int(rng.integers(17, 70)), int(rng.integers(17, 70))
            vol = oracle.gen_noise_ball(dims, np.dtype(dtype).itemsize, int(rng.integers(1 << 31)))
            if rng.integers(3) == 0:
                vol = rng.integers(0, 256 if dtype == np.uint8 else 4096, size=vol.shape).astype(dtype)
            vmin, vmax = int(vol.min()), int(vol.max())
            off = 1000 if dtype == np.uint16 else 0
            kind = rng.integers(4)
            stored = {0: vmin - 1, 1: vmax + 1}.get(int(kind), int(rng.integers(vmin, vmax + 1)))
            iso = stored - off
            view = ["front", "top", "bottom"][int(rng.integers(3))]
            filt, layout, accum, skip = (int(v) for v in rng.integers(2, size=4))
            use_tf = rng.integers(2) == 1
            lo, hi = (int(rng.integers(0, 40)), int(rng.integers(120, 256))) if dtype == np.uint8 else (int(rng.integers(-1000, 500)), int(rng.integers(1500, 3100)))
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
            r.setSkipEmpty(bool(skip))
            r.setTransferFunction(TF_ISO, TF_RGBA) if use_tf else r.setTransferFunction()
            r.setMIP(bool(rng.integers(2)))                      # ignored by the mode
            r.setIsosurface(True, iso)
            got = hip_iso(r)
            assert r.last_kernel_name == "raymarch_iso_kernel" and r.last_launch_choice == 0
            p = oracle.OracleParams(w, h, cam=cam, voxel_size=spacing, min_val=lo + off, max_val=hi + off, view_top=int(view == "top"),
                                    view_bottom=int(view == "bottom"), filter=filt, accum=accum,
                                    tf_rgba=r.getTransferLut() if use_tf else None)
            want = iso_ref.render(isolib, vol, p, iso)
            assert_same(got, want, f"case {case}: {dtype.__name__} {dims} {spacing} {w}x{h} iso {iso} {view} filt {filt} layout {layout} "
                                   f"accum {accum} skip {skip} tf {use_tf}")
            n_frames += 1
        assert n_frames == 150
    finally:
        r.close()


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
@pytest.mark.parametrize("stored", [2048, 4000, 5000])
def test_skipping_is_invisible_at_the_cfg2_shape(vra, oracle, cfg2, filt, stored):
    r = cfg2
    r.setFilter(filt)
    r.setCameraBlock(orbit_cam(oracle, 0.4, 0.6))
    r.setIsosurface(True, stored - 1000)
    frames = {}
    for skip in (False, True):
        r.setSkipEmpty(skip)
        frames[skip] = hip_iso(r)
    assert_same(frames[True], frames[False], f"skip on vs off, filter {filt}, stored iso {stored}")
    if stored < 4096:
        assert np.isfinite(frames[True][1]).any()


def _sampled_rows_match(r, vol, oracle, isolib, iso, rows, **kw):
    """the handle's last frame (rendered again for the counts) against the reference on `rows`"""
    w, h = r.framebuffer_size
    rgba = r.readPixels()
    depth = r.readDepth()
    _, spp = r.countSamples(per_pixel=True)
    for y in rows:
        want = iso_ref.render(isolib, vol, oracle.OracleParams(w, h, row_begin=y, row_end=y + 1, **kw), iso)
        assert_same((rgba[y:y + 1], depth[y:y + 1], spp[y:y + 1]), tuple(a[y:y + 1] for a in want), f"row {y}")


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


@pytest.mark.parametrize("filt,skip,stored,pose", [(0, True, 2048, 0), (1, True, 2048, 1), (1, False, 4000, 0), (0, False, 5000, 1)])
def test_cfg3_sampled_rows_match_the_reference(vra, oracle, isolib, cfg3, filt, skip, stored, pose):
    r, vol = cfg3
    cam = orbit_cam(oracle) if pose == 0 else orbit_cam(oracle, 0.5, 0.7)
    r.setCameraBlock(cam)
    r.setFilter(filt)
    r.setSkipEmpty(skip)
    r.setIsosurface(True, stored - 1000)
    r.render()
    _sampled_rows_match(r, vol, oracle, isolib, stored - 1000, (0, 333, 540, 1079), cam=cam, filter=filt, min_val=1000, max_val=1000)


@pytest.mark.parametrize("filt", [0, 1])
def test_2048_cubed_u8_sampled_rows_match_the_reference(vra, oracle, isolib, filt):
    R = vra.renderer
    with vra.RendererCore(0) as r:
        r.setup((960, 540))
        assert r.loadShader("VolumeRenderer.cs")
        r.setLayout(R.LAYOUT_BRICKED)
        r.generateSynthetic(R.SYNTH_NOISE_BALL, (2048, 2048, 2048), 1, 0x9E3779B9)
        vol = r.readVolume()                   # 8 GiB over PCIe
        cam = orbit_cam(oracle, 0.3, 0.4)
        r.setCameraBlock(cam)
        r.setFilter(filt)
        r.setSkipEmpty(True)
        r.setIsosurface(True, 128)
        r.render()
        _sampled_rows_match(r, vol, oracle, isolib, 128, (100, 270, 431), cam=cam, filter=filt, min_val=0, max_val=0)
        del vol


def _configure(r, vol, cam, filt, iso):
    r.setVolume(vol, (1.0, 1.2, 0.9))
    r.setCameraBlock(cam)
    r.setFilter(filt)
    r.setSkipEmpty(True)
    r.setIsosurface(True, iso)


@pytest.mark.parametrize("filt", [0, 1])
def test_row_shards_and_stripes_assemble_the_frame(vra, oracle, filt):
    vol = oracle.gen_noise_ball((61, 50, 47), 2, 5)
    cam = orbit_cam(oracle, 0.3, -0.5)
    size = (203, 157)
    with vra.RendererCore(0) as r:
        r.setup(size)
        assert r.loadShader("VolumeRenderer.cs")
        _configure(r, vol, cam, filt, 1500)
        full = hip_iso(r)
        # contiguous shards on the own (full-size) target
        for b, e in ((0, 50), (50, 120), (120, 157)):
            r.setRowRange(b, e)
            part = hip_iso(r)
            assert_same(tuple(a[b:e] for a in part), tuple(a[b:e] for a in full), f"rows [{b}, {e})")
        r.setRowRange(0, -1)
        # cyclic stripes of 16 rows, three ways
        for idx in range(3):
            r.setRowStripes(16, idx, 3)
            part = hip_iso(r)
            rows = [y for y in range(size[1]) if (y // 16) % 3 == idx]
            assert_same(tuple(a[rows] for a in part), tuple(a[rows] for a in full), f"stripe {idx}")
        r.setRowStripes(1, 0, 1)
    # a three-member group on device 0 (compact external targets, RGBA gather) assembles the same colour frame
    with vra.RendererGroup([0, 0, 0]) as g:
        g.setup(size, partition="stripes", stripe_rows=16)

        def conf(m):
            m.loadShader("VolumeRenderer.cs")
            _configure(m, vol, cam, filt, 1500)
        g.each(conf)
        g.render()
        got = g.readPixels()
    assert np.array_equal(bits(got), bits(full[0]))


def test_composite_iso_composite_leaks_no_state(vra, oracle, isolib):
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
        p = oracle.OracleParams(w, h, cam=cam, alpha_scale=0.3, min_val=10, max_val=200)
        want, _, want_spp = oracle.render(vol, p, want_spp=True)
        frames = []
        for step in range(3):
            r.setIsosurface(step == 1, 120)
            r.render()
            rgba = r.readPixels()
            _, spp = r.countSamples(per_pixel=True)
            if step == 1:
                assert r.last_kernel_name == "raymarch_iso_kernel"
                got = (rgba, r.readDepth(), spp)
                assert_same(got, iso_ref.render(isolib, vol, oracle.OracleParams(w, h, cam=cam, min_val=10, max_val=200), 120), "iso")
            else:
                assert r.last_kernel_name != "raymarch_iso_kernel"
                assert np.array_equal(bits(rgba), bits(want)) and np.array_equal(spp, want_spp), f"composite frame {step}"
    with vra.RendererCore(0) as fresh:
        fresh.setup((8, 8))
        with pytest.raises(vra.VRError) as e:
            fresh.readDepth()
        assert e.value.code == vra.renderer.VR_E_INVALID
