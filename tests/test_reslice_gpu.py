"""The multi-planar reslice kernel (vr_reslice.hip) against its CPU definition (tests/reslice_ref/reslice_ref.c): RGBA bits,
value bits and per-pixel sample counts, over a seeded matrix of small frames, the cfg3 and 2048^3 shapes on sampled rows, row
shards, stripes, compact and (grey, alpha) targets, a three-member group, mode round trips that must leave the composite and
isosurface frames and the measured launch choices untouched, and axis-aligned slabs against numpy directly."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("reslice_ref_binding", Path(__file__).resolve().parent / "reslice_ref" / "binding.py")
reslice_ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(reslice_ref)


@pytest.fixture(scope="session")
def rslib(tmp_path_factory):
    return reslice_ref.build(tmp_path_factory.mktemp("reslice_ref_gpu"))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(got, want, what):
    for name, g, w in zip(("rgba", "values", "count"), got, want):
        ok = np.array_equal(g, w) if name == "count" else np.array_equal(bits(g), bits(w))
        if not ok:
            bad = np.argwhere(bits(g) != bits(w)) if name != "count" else np.argwhere(g != w)
            y, x = bad[0][:2]
            raise AssertionError(f"{what}: {name} differs at {len(bad)} places, first (row {y}, col {x}): {g[y, x]} vs {w[y, x]}")


def hip_reslice(r):
    r.render()
    rgba = r.readPixels()
    values = r.readResliceValues()
    cnt = r.countSamples(per_pixel=True)[1]
    return rgba, values, cnt


def random_plane(vra, rng, dims, w, h, kind):
    """an oblique plane in voxel coordinates: kind 0 inside the volume, 1 partly outside, 2 wholly outside"""
    nx, ny, nz = dims
    big = float(max(dims))
    centre = np.array([nx - 1, ny - 1, nz - 1], dtype=np.float64) / 2.0 + rng.uniform(-0.15, 0.15, size=3) * np.array(dims)
    if kind == 2:
        centre = centre + rng.choice([-1.0, 1.0], size=3) * 3.0 * big
    pixel = (0.35 if kind == 0 else rng.uniform(1.0, 2.0)) * float(min(dims)) / float(max(w, h))
    step = float(rng.uniform(0.2, 2.0))
    return vra.reslice_geometry(dims, (1.0, 1.0, 1.0), centre, rng.normal(size=3), rng.normal(size=3), pixel, step, (w, h))


TF_ISO = [0, 60, 140, 255]
TF_RGBA = [[0.2, 0.9, 0.1, 0.0], [0.9, 0.3, 0.2, 0.4], [1.0, 0.8, 0.6, 0.8], [0.5, 0.5, 1.0, 1.0]]


def test_random_matrix_matches_the_reference(vra, oracle, rslib):
    R = vra.renderer
    rng = np.random.default_rng(20261016)
    r = vra.RendererCore(0)
    try:
        n_frames = 0
        for case in range(150):
            dtype = np.uint8 if rng.integers(2) == 0 else np.uint16
            dims = tuple(int(v) for v in rng.integers(9, 48, size=3))
            if case % 5 == 0:
                dims = (dims[0] | 1, dims[1], dims[2])          # nx % 4 != 0
            w, h = int(rng.integers(17, 70)), int(rng.integers(17, 70))
            vol = oracle.gen_noise_ball(dims, np.dtype(dtype).itemsize, int(rng.integers(1 << 31)))
            if rng.integers(3) == 0:
                vol = rng.integers(0, 256 if dtype == np.uint8 else 4096, size=vol.shape).astype(dtype)
            layout, filt = (int(v) for v in rng.integers(2, size=2))
            mode = ["mip", "minip", "mean"][case % 3]
            n = [1, 2, 7, 64][int(rng.integers(4))]
            kind = int(rng.integers(10))
            kind = 0 if kind < 4 else (1 if kind < 8 else 2)
            geom = random_plane(vra, rng, dims, w, h, kind)
            use_tf = rng.integers(2) == 1
            quirk_u16 = dtype == np.uint16 and rng.integers(3) != 0
            trunc = rng.integers(8) == 0
            off = 1000 if quirk_u16 else 0
            if rng.integers(6) == 0:
                lo = hi = int(rng.integers(0, 200))                 # max == min: every value windows to 0
            elif dtype == np.uint8:
                lo, hi = int(rng.integers(0, 40)), int(rng.integers(120, 256))
            else:
                lo, hi = int(rng.integers(-1000, 500)), int(rng.integers(1500, 3100))
            r.setup((w, h))
            assert r.loadShader("VolumeRenderer.cs")
            r.setQuirks((R.QUIRK_U16_OFFSET if quirk_u16 else 0) | (R.QUIRK_TRUNC_GRID if trunc else 0))
            r.setLayout(layout)
            r.setVolume(vol)
            r.setFilter(filt)
            r.setWindow(lo, hi)
            r.setSkipEmpty(bool(rng.integers(2)))                # no effect on reslice frames
            r.setMIP(bool(rng.integers(2)))                      # ignored by the mode
            r.setTransferFunction(TF_ISO, TF_RGBA) if use_tf else r.setTransferFunction()
            r.setReslice(True, geom, mode=mode, n=n)
            got = hip_reslice(r)
            assert r.last_kernel_name == "reslice_kernel" and r.last_launch_choice == 0
            want = reslice_ref.render(rslib, vol, geom, w, h, mode=mode, n=n, filt=filt, min_val=lo + off, max_val=hi + off,
                                      tf_rgba=r.getTransferLut() if use_tf else None, u16_offset=quirk_u16, trunc_grid=trunc)
            hl, wl = ((h // 16) * 16, (w // 16) * 16) if trunc else (h, w)
            assert_same(tuple(a[:hl, :wl] for a in got), tuple(a[:hl, :wl] for a in want),
                        f"case {case}: {dtype.__name__} {dims} {w}x{h} {mode} n {n} kind {kind} filt {filt} layout {layout} "
                        f"tf {use_tf} u16 quirk {quirk_u16} trunc {trunc} window [{lo}, {hi}]")
            r.setReslice(False)
            n_frames += 1
        assert n_frames == 150
    finally:
        r.close()


def _sampled_rows_match(r, vol, rslib, geom, rows, **kw):
    """rows rendered one at a time through setRowRange against the reference"""
    w, h = r.framebuffer_size
    for y in rows:
        r.setRowRange(y, y + 1)
        r.render()
        got = (r.readPixels()[y:y + 1], r.readResliceValues()[y:y + 1], r.countSamples(per_pixel=True)[1][y:y + 1])
        want = reslice_ref.render(rslib, vol, geom, w, h, row_begin=y, row_end=y + 1, **kw)
        assert_same(got, tuple(a[y:y + 1] for a in want), f"row {y}")
        assert got[2].sum() > 0, f"row {y} shows nothing"
    r.setRowRange(0, -1)


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


def _cfg3_plane(vra, oblique, w=1920, h=1080, dims=(1024, 1024, 1024)):
    if not oblique:
        return vra.axis_reslice("axial", 600, dims, (1.0, 1.0, 1.0), (w, h))
    c = np.array(dims, dtype=np.float64) / 2.0
    return vra.reslice_geometry(dims, (1.0, 1.0, 1.0), c, (0.0, -1.0, 1.0), (0.3, 1.0, 0.2), 0.9, 1.0, (w, h))


@pytest.mark.parametrize("oblique", [False, True])
@pytest.mark.parametrize("filt", [0, 1])
@pytest.mark.parametrize("mode", ["mip", "mean"])
def test_cfg3_sampled_rows_match_the_reference(vra, rslib, cfg3, oblique, filt, mode):
    r, vol = cfg3
    geom = _cfg3_plane(vra, oblique)
    r.setFilter(filt)
    r.setWindow(0, 3000)
    r.setReslice(True, geom, mode=mode, n=64)
    try:
        _sampled_rows_match(r, vol, rslib, geom, (0, 333, 540, 1079), mode=mode, n=64, filt=filt, min_val=1000, max_val=4000)
    finally:
        r.setReslice(False)


@pytest.mark.parametrize("filt", [0, 1])
def test_2048_cubed_u8_sampled_rows_match_the_reference(vra, rslib, filt):
    R = vra.renderer
    dims = (2048, 2048, 2048)
    with vra.RendererCore(0) as r:
        r.setup((960, 540))
        assert r.loadShader("VolumeRenderer.cs")
        r.setLayout(R.LAYOUT_BRICKED)
        r.generateSynthetic(R.SYNTH_NOISE_BALL, dims, 1, 0x9E3779B9)
        vol = r.readVolume()                   # 8 GiB over PCIe
        geom = vra.reslice_geometry(dims, (1.0, 1.0, 1.0), (1024.0, 1100.0, 1500.0), (0.2, -0.5, 1.0), (0.0, 1.0, 0.3), 2.3, 1.5, (960, 540))
        r.setFilter(filt)
        r.setWindow(0, 255)
        r.setReslice(True, geom, mode="mip", n=16)
        _sampled_rows_match(r, vol, rslib, geom, (100, 270, 431), mode="mip", n=16, filt=filt, min_val=0, max_val=255)
        del vol


def _configure(r, vol, geom, filt, mode, n, tf=False):
    r.setVolume(vol, (1.0, 1.2, 0.9))
    r.setFilter(filt)
    r.setWindow(-200, 2500)
    r.setTransferFunction(TF_ISO, TF_RGBA) if tf else r.setTransferFunction()
    r.setReslice(True, geom, mode=mode, n=n)


@pytest.mark.parametrize("filt,mode,tf", [(0, "mip", False), (1, "mean", False), (1, "minip", True)])
def test_shards_stripes_and_targets_assemble_the_frame(vra, oracle, filt, mode, tf):
    import torch

    R = vra.renderer
    sharding = __import__("importlib").import_module("volume-renderer_amd.sharding")
    vol = oracle.gen_noise_ball((61, 50, 47), 2, 5)
    size = (203, 157)
    geom = vra.reslice_geometry((61, 50, 47), (1, 1, 1), (30.0, 24.0, 23.0), (0.3, 0.4, 1.0), (0.0, 1.0, 0.0), 0.45, 0.8, size)
    with vra.RendererCore(0) as r:
        r.setup(size)
        assert r.loadShader("VolumeRenderer.cs")
        _configure(r, vol, geom, filt, mode, 7, tf)
        full = hip_reslice(r)
        assert full[2].sum() > 0 and (full[2] == 0).sum() > 0
        # contiguous shards on the own (full-size) target
        for b, e in ((0, 50), (50, 120), (120, 157)):
            r.setRowRange(b, e)
            part = hip_reslice(r)
            assert_same(tuple(a[b:e] for a in part), tuple(a[b:e] for a in full), f"rows [{b}, {e})")
        r.setRowRange(0, -1)
        # cyclic stripes of 16 rows, three ways
        for idx in range(3):
            r.setRowStripes(16, idx, 3)
            part = hip_reslice(r)
            rows = [y for y in range(size[1]) if (y // 16) % 3 == idx]
            assert_same(tuple(a[rows] for a in part), tuple(a[rows] for a in full), f"stripe {idx}")
        r.setRowStripes(1, 0, 1)
        # compact external target: rows 40..103 land at local rows 0..63, values indexed like it
        w, h = size
        tgt = torch.zeros((64, w, 4), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        r.setFramebufferExternal(tgt.data_ptr())
        r.setFramebufferCompact(True)
        r.setRowRange(40, 104)
        r.render()
        r.synchronize()
        assert np.array_equal(bits(tgt.cpu().numpy()), bits(full[0][40:104]))
        assert np.array_equal(bits(r.readResliceValues(rows=64)), bits(full[1][40:104]))
        r.setRowRange(0, -1)
        r.setFramebufferCompact(False)
        # (grey, alpha) target: grey modes only
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
            _configure(m, vol, geom, filt, mode, 7, tf)
        g.each(conf)
        g.render()
        got = g.readPixels()
    assert np.array_equal(bits(got), bits(full[0]))


def test_composite_reslice_composite_leaves_the_composite_frames_and_choices(vra, oracle, rslib):
    vol = oracle.gen_noise_ball((40, 36, 44), 1, 9)
    w, h = 97, 83
    geom = vra.axis_reslice("coronal", 20, (40, 36, 44), (1, 1, 1), (w, h), n=5)
    with vra.RendererCore(0) as r:
        r.setup((w, h))
        assert r.loadShader("VolumeRenderer.cs")
        r.setVolume(vol)
        r.setWindow(10, 200)
        r.setAlpha(0.3)
        r.setSkipEmpty(True)
        r.setAutotune(True)
        frames = []
        blobs = []
        for step in range(3):
            if step == 1:
                blobs.append(r.exportChoices())
                r.setReslice(True, geom, mode="mean", n=5)
            else:
                r.setReslice(False)
            r.render()
            rgba = r.readPixels()
            _, spp = r.countSamples(per_pixel=True)
            if step == 1:
                assert r.last_kernel_name == "reslice_kernel" and r.last_launch_choice == 0
                got = (rgba, r.readResliceValues(), spp)
                assert_same(got, reslice_ref.render(rslib, vol, geom, w, h, mode="mean", n=5, min_val=10, max_val=200), "reslice")
                blobs.append(r.exportChoices())
            else:
                assert r.last_kernel_name != "reslice_kernel"
                frames.append((rgba, spp))
        assert np.array_equal(bits(frames[0][0]), bits(frames[1][0])) and np.array_equal(frames[0][1], frames[1][1])
        assert blobs[0] == blobs[1]


def test_iso_reslice_iso_keeps_the_iso_frames_and_depth(vra, oracle):
    vol = oracle.gen_noise_ball((40, 36, 44), 2, 19)
    w, h = 90, 70
    geom = vra.axis_reslice("sagittal", 17, (40, 36, 44), (1, 1, 1), (w, h))
    with vra.RendererCore(0) as r:
        r.setup((w, h))
        assert r.loadShader("VolumeRenderer.cs")
        r.setVolume(vol)
        r.setWindow(0, 3000)
        r.setIsosurface(True, 1200)
        r.render()
        iso0 = (r.readPixels(), r.readDepth())
        r.setIsosurface(False, 1200)
        r.setReslice(True, geom, mode="mip", n=3)
        r.render()
        assert r.last_kernel_name == "reslice_kernel"
        assert np.array_equal(bits(r.readDepth()), bits(iso0[1]))          # a reslice frame leaves the depth target alone
        r.setReslice(False)
        r.setIsosurface(True, 1200)
        r.render()
        assert r.last_kernel_name == "raymarch_iso_kernel"
        assert np.array_equal(bits(r.readPixels()), bits(iso0[0])) and np.array_equal(bits(r.readDepth()), bits(iso0[1]))
    with vra.RendererCore(0) as fresh:
        fresh.setup((8, 8))
        with pytest.raises(vra.VRError) as e:
            fresh.readResliceValues()
        assert e.value.code == vra.renderer.VR_E_INVALID


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("layout", [0, 1])
def test_axis_aligned_slabs_are_numpy_max_min_and_mean(vra, dtype, layout):
    """independent of the reference: a z slab of 2m + 1 voxels renders numpy's reductions of vol[k - m : k + m + 1]"""
    R = vra.renderer
    rng = np.random.default_rng(7 + layout)
    vol = rng.integers(0, 256 if dtype == np.uint8 else 4096, size=(33, 27, 38)).astype(dtype)
    nz, ny, nx = vol.shape
    k, m = 16, 4
    slab = vol[k - m:k + m + 1].astype(np.float32)
    acc = np.zeros((ny, nx), dtype=np.float32)
    for s in slab:
        acc = (acc + s).astype(np.float32)
    want = {"mip": slab.max(0), "minip": slab.min(0), "mean": acc / np.float32(2 * m + 1)}
    off = np.float32(1000.0) if dtype == np.uint16 else np.float32(0.0)
    with vra.RendererCore(0) as r:
        r.setup((nx, ny))
        assert r.loadShader("VolumeRenderer.cs")
        r.setLayout(layout)
        r.setVolume(vol)
        r.setWindow(0, 255 if dtype == np.uint8 else 3095)
        for filt in (0, 1):
            r.setFilter(filt)
            for mode, v in want.items():
                r.setReslice(True, vra.axis_reslice("axial", k, (nx, ny, nz), (1, 1, 1), (nx, ny), n=2 * m + 1), mode=mode, n=2 * m + 1)
                r.render()
                assert r.countSamples() == nx * ny * (2 * m + 1)
                assert np.array_equal(bits(r.readResliceValues()), bits(v - off)), (mode, filt)
                lo = np.float32(1000.0) if dtype == np.uint16 else np.float32(0.0)
                hi = np.float32(4095.0) if dtype == np.uint16 else np.float32(255.0)
                grey = ((np.minimum(np.maximum(v, lo), hi) - lo) / (hi - lo)).astype(np.float32)
                assert np.array_equal(bits(r.readPixels()[..., 0]), bits(grey)), (mode, filt)
        r.setReslice(False)
