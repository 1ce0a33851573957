"""The isosurface, reslice and shading kernels at the sampler's edges (tests/edge_cases.py): thin volumes, the first and the last
voxel of the buffer, cameras inside / grazing / far, images smaller than a tile, zero gradients, max == min, the +1000 quirk, the
truncated grid, the 10 000-step budget, the tail of the reslice loop and iso values that meet a stored value exactly.

vr_iso.hip, vr_reslice.hip and vr_shade.hip share one sampler (csrc/vr_sampler.h), iso and shade also the ray start and the skip
cell (csrc/vr_march.h), but each wraps its own march loop, gradient and reduction around them; the composite kernels' edge tests (the tiny volumes of test_parity_gpu.py) do not reach them.  Every
comparison is against the mode's CPU definition (tests/iso_ref, tests/reslice_ref, tests/shade_ref; tests/test_mode_edges_cpu.py
anchors those at the same edges) on every output the mode has -- RGBA bits, per-pixel counts, depth bits, reslice value bits.
Windows and iso values are in STORED units and the handles run with setQuirks(0), unless a case says that it converts through
the +1000 of VR_QUIRK_U16_OFFSET.
"""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_HERE = Path(__file__).resolve().parent


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


iso_ref = _load("iso_ref_binding", _HERE / "iso_ref" / "binding.py")
reslice_ref = _load("reslice_ref_binding", _HERE / "reslice_ref" / "binding.py")
shade_ref = _load("shade_ref_binding", _HERE / "shade_ref" / "binding.py")
E = _load("edge_cases", _HERE / "edge_cases.py")

KERNELS = {"iso": "raymarch_iso_kernel", "reslice": "reslice_kernel", "shade": "raymarch_shade_kernel"}
OUTPUTS = {"iso": ("rgba", "depth", "spp"), "reslice": ("rgba", "values", "count"), "shade": ("rgba", "spp")}
FILTERS = pytest.mark.parametrize("filt", [0, 1], ids=["nearest", "trilinear"])
MODES = pytest.mark.parametrize("mode", ["iso", "shade", "reslice"])


@pytest.fixture(scope="session")
def refs(tmp_path_factory):
    d = tmp_path_factory.mktemp("mode_edges_refs_gpu")
    return {"iso": (iso_ref, iso_ref.build(d)), "shade": (shade_ref, shade_ref.build(d)), "reslice": (reslice_ref, reslice_ref.build(d))}


@pytest.fixture
def handle(vra):
    r = vra.RendererCore(0)
    yield r
    r.close()


def assert_same(mode, got, want, what, region=None):
    """every output of the mode, float32 arrays by their bits; region: (rows, cols) index of the rendered part"""
    for name, g, w in zip(OUTPUTS[mode], got, want):
        if region is not None:
            g, w = g[region[0]][:, region[1]], w[region[0]][:, region[1]]
        bad = (g != w) if name in ("spp", "count") else (E.bits(g) != E.bits(w))
        if bad.any():
            at = tuple(int(i) for i in np.argwhere(bad)[0])
            raise AssertionError(f"{what}: {name} differs at {int(bad.sum())} places, first {at}: {g[at]} vs {w[at]}")


def load(r, size, vol, spacing=(1.0, 1.0, 1.0), layout=0, quirks=0):
    r.setup(size)
    assert r.loadShader("VolumeRenderer.cs")
    r.setQuirks(quirks)
    r.setLayout(layout)
    r.setVolume(vol, spacing)
    r.setRowRange(0, -1)
    r.setRowStripes(1, 0, 1)


def view_and_window(r, filt, win, view="front", cam=None, tf=False, skip=False, accum=0):
    r.setFilter(filt)
    r.setAccum(accum)
    r.setWindow(*win)
    r.setSkipEmpty(bool(skip))
    r.setInitialCameraRotation(view == "top", view == "bottom")
    if cam is not None:
        r.setCameraBlock(cam)
    r.setTransferFunction(E.TF_ISO, E.TF_RGBA) if tf else r.setTransferFunction()
    return r.getTransferLut() if tf else None


def render(r, mode):
    r.render()
    assert r.last_kernel_name == KERNELS[mode], r.last_kernel_name
    rgba = r.readPixels()
    spp = r.countSamples(per_pixel=True)[1]
    assert r.last_kernel_name == KERNELS[mode], r.last_kernel_name
    if mode == "iso":
        return rgba, r.readDepth(), spp
    if mode == "reslice":
        return rgba, r.readResliceValues(), spp
    return rgba, spp


def params(oracle, size, cam, spacing, view, filt, **kw):
    return oracle.OracleParams(size[0], size[1], cam=cam, voxel_size=spacing, view_top=int(view == "top"), view_bottom=int(view == "bottom"),
                               filter=filt, **kw)


# ---------------------------------------------------------------------------------------------------------------
# 1: thin volumes, the first and the last voxel, random cameras
# ---------------------------------------------------------------------------------------------------------------
@MODES
@FILTERS
@pytest.mark.parametrize("dtype", E.DTYPES, ids=["u8", "u16"])
def test_thin_volumes_read_the_first_and_last_voxel(vra, oracle, refs, handle, mode, filt, dtype):
    """the seeded frames of edge_cases.thin_cases on `corners` volumes of the whole pool; test_mode_edges_cpu.py shows that more
    than half of them change with the last voxel of the buffer and more than half with the first.  (The x-pair load of the last
    voxel reaches past the buffer, and a partly out-of-range buffer load returns 0 for all of it: the composite kernels'
    test_trilinear_on_tiny_volumes_reads_the_last_voxel, for the three other kernels.)  One voxel type per test, to keep each
    one shorter than the existing random matrices."""
    r = handle
    frames = shown = 0
    for g in E.thin_cases(mode, filt):
        if g.dtype != dtype:
            continue
        for case in g.cases:
            load(r, E.THIN_SIZE, g.vol, case.spacing, case.layout)
            lut = view_and_window(r, filt, E.thin_window(case.dtype), case.view, case.cam, case.tf, case.skip)
            if mode == "iso":
                r.setIsosurface(True, E.thin_iso(case.dtype))
            elif mode == "shade":
                r.setAlpha(E.THIN_ALPHA)
                r.setMIP(False)
                r.setShading(True, *case.coef)
            else:
                r.setReslice(True, case.geom, mode=case.red, n=case.n)
            got = render(r, mode)
            want = E.thin_reference(refs, oracle, mode, case, filt, lut, g.vol)
            assert_same(mode, got, want, case.what)
            if mode == "reslice":
                r.setReslice(False)
            frames += 1
            shown += int(want[-1].any())
    assert frames == len(E.DIMS_POOL) * E.CAMERAS_PER_VOLUME and shown >= frames // 2, (frames, shown)


# ---------------------------------------------------------------------------------------------------------------
# 2: zero gradients
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["iso", "shade"])
@FILTERS
def test_zero_gradients_give_hits_and_no_nan(vra, oracle, refs, handle, mode, filt):
    """`constant` volumes of the whole pool and 1 x 1 x 1 volumes: every central difference is 0 and the normal falls back to -dir"""
    r = handle
    rng = np.random.default_rng(20261240 + filt)
    opt = np.random.default_rng(20261245 + filt)                       # the settings of a frame: drawn, so tied to no loop
    coefs = [E.COEFS[2], E.COEFS[3], E.COEFS[0], E.COEFS[4]]           # shininess 1, 128, 16, 2
    seen = set()
    hits = k = 0
    for dims in E.DIMS_POOL + [(1, 1, 1)]:
        for dtype in E.DTYPES:
            vol = E.make_volume(rng, "constant", dims, dtype)
            value, vmax = int(vol.flat[0]), E.vmax_of(dtype)
            for c in range(2):
                size = E.pick(opt, (E.THIN_SIZE, (33, 21)))
                spacing, view = E.pick(opt, E.SPACINGS), E.pick(opt, E.VIEWS)
                layout, skip, tf, below = (E.pick(opt, (0, 1)) for _ in range(4))
                seen.add((np.dtype(dtype).name, layout, skip))
                cam = E.random_camera_block(rng, 0.0, 2.5)
                load(r, size, vol, spacing, layout)
                lut = view_and_window(r, filt, (0, vmax), view, cam, tf, skip)
                p = params(oracle, size, cam, spacing, view, filt, min_val=0, max_val=vmax, alpha_scale=0.3, tf_rgba=lut)
                what = f"{mode} filt {filt} {dims} {np.dtype(dtype).name} value {value} {size} {spacing} {view} layout {layout} skip {skip} tf {tf}"
                if mode == "iso":
                    iso = value - below
                    r.setIsosurface(True, iso)
                    want = iso_ref.render(refs["iso"][1], vol, p, iso, u16_offset=False)
                    hit = np.isfinite(want[1])
                else:
                    coef = coefs[k % len(coefs)]
                    r.setAlpha(0.3)
                    r.setMIP(False)
                    r.setShading(True, *coef)
                    want = shade_ref.render(refs["shade"][1], vol, p, *coef)
                    hit = want[0][..., 3] > 0
                    what += f" coef {coef}"
                got = render(r, mode)
                assert not np.isnan(got[0]).any(), what
                assert_same(mode, got, want, what)
                if mode == "iso":
                    assert np.array_equal(np.isfinite(got[1]), hit), what
                    assert tf or np.all(got[0][hit][:, :3] > 0.99), what                  # white, lit head-on
                hits += int(hit.sum())
                k += 1
    assert hits > 10000, hits
    assert len(seen) == 8, seen                     # (voxel type, layout, skip): all eight


# ---------------------------------------------------------------------------------------------------------------
# 3: images smaller than a tile, the truncated grid, row ranges and stripes
# ---------------------------------------------------------------------------------------------------------------
def small_image_case(vra, oracle, refs, r, rng, opt, mode, filt, dims, dtype, size):
    """configures the handle for one frame of the matrix (its settings drawn from `opt`); returns (reference(trunc, rows) -> frame,
    what, (layout, skip, tf))"""
    vol = E.make_volume(rng, "random", dims, dtype)
    spacing, view = E.pick(opt, E.SPACINGS), E.pick(opt, E.VIEWS)
    layout, skip, tf = (E.pick(opt, (0, 1)) for _ in range(3))
    lo, hi = E.thin_window(dtype)
    what = f"{mode} filt {filt} {dims} {np.dtype(dtype).name} {size} layout {layout} skip {skip} tf {tf}"
    if mode == "reslice":
        n, red = E.pick(opt, (1, 3, 6)), E.pick(opt, E.REDUCTIONS)
        geom = E.corner_plane(rng, dims, (max(size[0], 8), max(size[1], 8)), n)
        load(r, size, vol, spacing, layout)
        lut = view_and_window(r, filt, (lo, hi), tf=tf)
        r.setReslice(True, geom, mode=red, n=n)

        def reference(trunc=False, rows=(0, -1)):
            return reslice_ref.render(refs["reslice"][1], vol, geom, size[0], size[1], mode=red, n=n, filt=filt, min_val=lo, max_val=hi, tf_rgba=lut,
                                      u16_offset=False, trunc_grid=trunc, row_begin=rows[0], row_end=rows[1])
        return reference, what + f" {red} n {n}", (layout, skip, tf)
    cam = E.random_camera_block(rng, 0.0, 3.0)
    load(r, size, vol, spacing, layout)
    lut = view_and_window(r, filt, (lo, hi), view, cam, tf, skip)
    if mode == "iso":
        iso = int(np.sort(vol.reshape(-1))[vol.size // 2])
        r.setIsosurface(True, iso)
    else:
        coef = E.pick(opt, E.COEFS)
        r.setAlpha(0.3)
        r.setMIP(False)
        r.setShading(True, *coef)

    def reference(trunc=False, rows=(0, -1)):
        p = params(oracle, size, cam, spacing, view, filt, min_val=lo, max_val=hi, alpha_scale=0.3, tf_rgba=lut, trunc_grid=int(trunc),
                   row_begin=rows[0], row_end=rows[1])
        if mode == "iso":
            return iso_ref.render(refs["iso"][1], vol, p, iso, u16_offset=False)
        return shade_ref.render(refs["shade"][1], vol, p, *coef)
    return reference, what + f" {spacing} {view}", (layout, skip, tf)


@MODES
@FILTERS
def test_small_images_and_the_truncated_grid(vra, oracle, refs, handle, mode, filt):
    """1 x 1 to 68 x 68: less than a wavefront's 8 x 8 patch, less than a 16 x 16 tile, one tile exactly, tiles with a remainder.
    With VR_QUIRK_TRUNC_GRID only whole tiles are rendered and only they are compared.  On 68 x 68 and 15 x 17 also a row range and
    cyclic stripes whose first row is no multiple of 16."""
    R = vra.renderer
    r = handle
    rng = np.random.default_rng(20261250 + filt)
    opt = np.random.default_rng(20261255 + filt)
    seen = set()
    k = shown = 0
    for dims in ((9, 5, 4), (2, 3, 5)):
        for size in E.IMAGE_SIZES:
            dtype = E.DTYPES[(k + k // len(E.IMAGE_SIZES)) % 2]          # either type at every size
            reference, what, settings = small_image_case(vra, oracle, refs, r, rng, opt, mode, filt, dims, dtype, size)
            seen.add(settings[:2])
            w, h = size
            want = reference()
            assert_same(mode, render(r, mode), want, what)
            shown += int(want[-1].any())
            # whole tiles only
            r.setQuirks(R.QUIRK_TRUNC_GRID)
            region = (slice(0, (h // 16) * 16), slice(0, (w // 16) * 16))
            assert_same(mode, render(r, mode), reference(trunc=True), what + " truncated grid", region)
            r.setQuirks(0)
            if size in ((68, 68), (15, 17)):
                b, e = (5, 41) if h == 68 else (3, 13)
                r.setRowRange(b, e)
                assert_same(mode, render(r, mode), reference(rows=(b, e)), what + f" rows [{b}, {e})", (slice(b, e), slice(0, w)))
                r.setRowRange(0, -1)
                r.setRowStripes(8, 1, 3)                         # rows 8..15, 32..39, 56..63
                rows = np.array([y for y in range(h) if (y // 8) % 3 == 1])
                assert_same(mode, render(r, mode), want, what + " stripes of 8 rows, 1 of 3", (rows, slice(0, w)))
                r.setRowStripes(1, 0, 1)
            if mode == "reslice":
                r.setReslice(False)
            k += 1
    assert shown >= 12, shown
    assert len(seen) == 4, seen                     # (layout, skip): all four


# ---------------------------------------------------------------------------------------------------------------
# 4: max == min and the +1000 of 16-bit volumes, isosurface and shading
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["iso", "shade"])
@FILTERS
def test_degenerate_window_and_the_u16_offset(vra, oracle, refs, handle, mode, filt):
    """lo == hi (every sample windows to 0; with a transfer function: to its entry 0) and ordinary windows; on half of the 16-bit
    cases VR_QUIRK_U16_OFFSET is on, the window and the iso value go in 1000 lower and the reference converts them back"""
    R = vra.renderer
    r = handle
    rng = np.random.default_rng(20261260 + filt)
    opt = np.random.default_rng(20261265 + filt)
    size = (40, 33)
    seen = set()
    hits = k = 0
    for di, dims in enumerate(E.DIMS_POOL):
        for dtype in E.DTYPES:
            vol = E.make_volume(rng, "random", dims, dtype)
            vmax = E.vmax_of(dtype)
            for ci, (degenerate, tf) in enumerate(((1, 0), (1, 1), (0, 0), (0, 1))):
                quirk = dtype == np.uint16 and (ci + ci // 2 + di) % 2 == 1          # half of the 16-bit frames, in every combination
                seen.add((np.dtype(dtype).name, degenerate, tf, quirk))
                off = 1000 if quirk else 0
                lo = int(rng.integers(0, vmax // 3))
                hi = lo if degenerate else int(rng.integers(vmax // 2, vmax + 1))
                spacing, view, layout, skip = E.pick(opt, E.SPACINGS), E.pick(opt, E.VIEWS), E.pick(opt, (0, 1)), E.pick(opt, (0, 1))
                cam = E.random_camera_block(rng, 0.0, 3.0)
                load(r, size, vol, spacing, layout, R.QUIRK_U16_OFFSET if quirk else 0)
                lut = view_and_window(r, filt, (lo - off, hi - off), view, cam, tf, skip)
                p = params(oracle, size, cam, spacing, view, filt, min_val=lo, max_val=hi, alpha_scale=1.0, tf_rgba=lut)
                what = (f"{mode} filt {filt} {dims} {np.dtype(dtype).name} window [{lo}, {hi}] quirk {quirk} tf {tf} {spacing} {view} layout {layout} "
                        f"skip {skip}")
                if mode == "iso":
                    iso = int(np.sort(vol.reshape(-1))[(vol.size * 3) // 4])
                    r.setIsosurface(True, iso - off)
                    want = iso_ref.render(refs["iso"][1], vol, p, iso - off, u16_offset=quirk)
                    hits += int(np.isfinite(want[1]).sum())
                else:
                    coef = E.pick(opt, E.COEFS)
                    r.setAlpha(1.0)
                    r.setMIP(False)
                    r.setShading(True, *coef)
                    want = shade_ref.render(refs["shade"][1], vol, p, *coef)
                    hits += int((want[0][..., 3] > 0).sum())
                    if degenerate:
                        assert not want[0].any(), what
                got = render(r, mode)
                assert_same(mode, got, want, what)
                k += 1
    assert hits > 5000, hits
    # lo == hi with and without a transfer function, ordinary windows likewise; 16-bit volumes with the +1000 on and off in each
    assert seen == {(t, d, f, q) for t, qs in (("uint8", (False,)), ("uint16", (False, True))) for d in (0, 1) for f in (0, 1) for q in qs}, seen


# ---------------------------------------------------------------------------------------------------------------
# 5: the step budget
# ---------------------------------------------------------------------------------------------------------------
BUDGET_DIMS = (16384, 2, 2)                      # the shape of test_parity_gpu.py::test_step_budget_of_10000_samples
BUDGET_SPACING = (1.0, 4096.0, 4096.0)           # a box of 1 x 0.5 x 0.5 with a step of 7.5e-5: 13 000 steps along x
BUDGET_SIZE = (24, 16)
# two of that test's three poses: on this image the reference's largest count at its third, (-0.9, 0.7), is 9840, and the cap is the point
BUDGET_POSES = ((0.0, 2.244), (0.3, 2.1))


@pytest.mark.parametrize("mode", ["iso", "shade"])
def test_step_budget_of_10000_samples(vra, oracle, refs, handle, mode):
    """Q6: the march takes at most 10 000 samples.  The isosurface with its value above every voxel (skipping off and on: the
    skipped steps count) and the shaded composite at an opacity too small to terminate both run into the cap.  (The pose
    (-0.9, 0.7) of the composite test is left out: its rays cross the box at an angle and the reference peaks at 9840 there.)"""
    r = handle
    rng = np.random.default_rng(10000)
    vol = rng.integers(0, 256, size=BUDGET_DIMS[::-1], dtype=np.uint8)
    capped = 0
    for pi, (ze, az) in enumerate(BUDGET_POSES):
        c = oracle.Camera()
        c.orient(0.0, ze, az)
        cam = c.block()
        p = params(oracle, BUDGET_SIZE, cam, BUDGET_SPACING, "front", 0, min_val=0, max_val=255, alpha_scale=0.00005)
        if mode == "iso":
            want = iso_ref.render(refs["iso"][1], vol, p, 256, u16_offset=False)
        else:
            want = shade_ref.render(refs["shade"][1], vol, p, *E.COEFS[0])
        assert int(want[-1].max()) == 10000, (ze, az, int(want[-1].max()))
        capped += int((want[-1] == 10000).sum())
        for skip in ((False, True) if mode == "iso" else (False,)):
            load(r, BUDGET_SIZE, vol, BUDGET_SPACING, (pi + int(skip)) % 2)           # either layout with and without skipping
            view_and_window(r, 0, (0, 255), cam=cam, skip=skip)
            if mode == "iso":
                r.setIsosurface(True, 256)
            else:
                r.setAlpha(0.00005)
                r.setMIP(False)
                r.setShading(True, *E.COEFS[0])
            got = render(r, mode)
            assert_same(mode, got, want, f"{mode} 10000-step cap pose ({ze}, {az}) skip {skip}")
            assert int(got[-1].max()) == 10000
    assert capped >= 30, capped


# ---------------------------------------------------------------------------------------------------------------
# 6: the tail of the reslice loop
# ---------------------------------------------------------------------------------------------------------------
@FILTERS
def test_reslice_slab_tails_on_thin_volumes(vra, oracle, refs, handle, filt):
    """n = 1..9, 1023 and 1024 on 2 x 3 x 5 and 5 x 1 x 3: the loop is unrolled by 4, the lanes of its last round with k >= n sample
    voxel 0 and must not be taken.  Oblique planes through both corner voxels with a margin outside the volume, so the counts vary
    within the frame; from n = 8 on the slabs are longer than the volume's diagonal, so every one of them has samples outside."""
    r = handle
    rng = np.random.default_rng(20261270 + filt)
    k = 0
    for dims in ((2, 3, 5), (5, 1, 3)):
        diag = float(np.linalg.norm(dims))
        for n in list(range(1, 10)) + [1023, 1024]:
            size = (29, 23) if n < 1000 else (17, 13)                      # (the long slabs on smaller frames: the reference's time)
            for red in E.REDUCTIONS:
                dtype, layout = E.DTYPES[k % 2], (k // 2) % 2
                vol = E.make_volume(rng, ("random", "corners")[(k // 3) % 2], dims, dtype)
                step = float(rng.uniform(0.3, 1.0))
                if n >= 8:
                    step = max(step, 1.2 * diag / n)
                geom = E.corner_plane(rng, dims, size, n, step)
                lo, hi = E.thin_window(dtype)
                load(r, size, vol, layout=layout)
                lut = view_and_window(r, filt, (lo, hi), tf=k % 4 == 3)
                r.setReslice(True, geom, mode=red, n=n)
                what = f"reslice filt {filt} {dims} {np.dtype(dtype).name} n {n} {red} layout {layout} step {step:.4f}"
                want = reslice_ref.render(refs["reslice"][1], vol, geom, size[0], size[1], mode=red, n=n, filt=filt, min_val=lo, max_val=hi,
                                          tf_rgba=lut, u16_offset=False)
                cnt = want[2]
                assert len(np.unique(cnt)) >= 2 and cnt.max() > 0, (what, np.unique(cnt))
                assert n < 8 or cnt.max() < n, (what, int(cnt.max()))
                assert_same("reslice", render(r, "reslice"), want, what)
                r.setReslice(False)
                k += 1
    assert k == 66


# ---------------------------------------------------------------------------------------------------------------
# 7: edge iso values
# ---------------------------------------------------------------------------------------------------------------
@FILTERS
def test_iso_value_at_or_below_the_minimum_hits_on_the_first_sample_from_inside(vra, oracle, refs, handle, filt):
    """the eye inside the box, the iso value at the data minimum or one below: every ray hits at sample 0, where the refinement
    has no sample before it (h = q_0)"""
    r = handle
    rng = np.random.default_rng(20261280 + filt)
    size = (33, 27)
    k = 0
    for dims in E.DIMS_POOL:
        dtype = E.DTYPES[k % 2]
        vol = E.make_volume(rng, "random", dims, dtype)
        for c in range(2):
            spacing, view, layout, skip = E.SPACINGS[k % 2], E.VIEWS[k % 3], (k // 2) % 2, c
            cam = E.random_camera_block(rng, 0.0, 0.02)                  # every box here is at least 0.04 thick
            iso = int(vol.min()) - (k + c) % 2
            load(r, size, vol, spacing, layout)
            lut = view_and_window(r, filt, E.thin_window(dtype), view, cam, c == 1, skip)
            r.setIsosurface(True, iso)
            p = params(oracle, size, cam, spacing, view, filt, min_val=E.thin_window(dtype)[0], max_val=E.thin_window(dtype)[1], tf_rgba=lut)
            want = iso_ref.render(refs["iso"][1], vol, p, iso, u16_offset=False)
            what = f"iso filt {filt} {dims} {np.dtype(dtype).name} iso {iso} {spacing} {view} layout {layout} skip {skip}"
            assert np.all(want[2] == 1) and np.all(np.isfinite(want[1])), what       # inside: every ray marches, and hits at once
            assert_same("iso", render(r, "iso"), want, what)
        k += 1


@FILTERS
def test_iso_value_equal_to_a_stored_value_is_a_hit(vra, oracle, refs, handle, filt):
    """the iso value is the largest value of the `corners` background: voxels that hold exactly it are hits (s >= iso), and only
    the two corner voxels lie above it.  Under NEAREST the reference's frame at iso + 1 is the frame a `>` would give: it must
    differ, or the case shows nothing."""
    r = handle
    rng = np.random.default_rng(20261290 + filt)
    size = (48, 40)
    visible = k = 0
    for dims in E.DIMS_POOL[1:]:
        for dtype in E.DTYPES:
            vol = E.make_volume(rng, "corners", dims, dtype)
            iso = int(np.sort(vol.reshape(-1))[-3]) if vol.size > 2 else int(vol.max())
            spacing, view, layout, skip = E.SPACINGS[k % 2], E.VIEWS[k % 3], (k // 2) % 2, (k // 3) % 2
            cam = E.random_camera_block(rng)
            load(r, size, vol, spacing, layout)
            lut = view_and_window(r, filt, E.thin_window(dtype), view, cam, k % 4 == 2, skip)
            r.setIsosurface(True, iso)
            p = params(oracle, size, cam, spacing, view, filt, min_val=E.thin_window(dtype)[0], max_val=E.thin_window(dtype)[1], tf_rgba=lut)
            want = iso_ref.render(refs["iso"][1], vol, p, iso, u16_offset=False)
            what = f"iso filt {filt} {dims} {np.dtype(dtype).name} iso {iso} {spacing} {view} layout {layout} skip {skip}"
            assert_same("iso", render(r, "iso"), want, what)
            visible += int(bool(E.differ(want, iso_ref.render(refs["iso"][1], vol, p, iso + 1, u16_offset=False))))
            k += 1
    assert filt == 1 or visible >= k // 2, (visible, k)
