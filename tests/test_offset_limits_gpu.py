"""Every kernel that reads the volume, at the limits of 32-bit voxel offsets (tests/offset_limits.py restates the host's predicate
and holds the shapes; tests/test_offset_limits_cpu.py pins each shape to its side).

1. Both sides of every stride threshold on volumes of 32 to 128 MiB: the factor in question is the largest the 24-bit multiplies of
   the 32-bit path may see, and its neighbour runs the 64-bit instances -- of every kernel and mode, the fast kernel's 64-bit address
   tables included -- in seconds.  The side is asserted from the restated predicate and through the dispatcher: kernel variant 3
   runs raymarch_relay_kernel on the headline mode only with 32-bit offsets, raymarch_fast_kernel otherwise.
2. The 32-bit path with bit 31 of the offset set, on the smallest volumes that set it (2 GiB and the 4 GiB top of the path).

References: oracle.render, tests/iso_ref, tests/reslice_ref, tests/shade_ref.  Frames, per-pixel sample counts, depth and reslice
values are compared bit for bit.  48 tests, 10 to 12 s on an MI355X for the whole file (the 2 to 4 GiB volumes are generated on the device
and read back once each: 0.3 to 2 s of set-up per volume).

What catches what (checked once by hand on copies of the library, nothing of it kept): the 32-bit offset masked to 31 bits in
VoxelFetch<..., false>::load and VolumeSampler::tap2 fails all 16 tests of part 2 and nothing else; bstride_z masked to 23 bits in
buildFrame fails the six 32-bit `bstride_z` tests of part 1 and the eight tests of part 2 on the 8-bit volumes (bricked); `<=` for
`<` on ny * nz fails the two NEAREST tests on the 64-bit side of `ny*nz`, by the kernel that ran.  The suite as it was passes under
the first two.

Not here: the staged TRILINEAR kernel's 2^31-byte limit on relative offsets (csrc/vr_tslab.hip, "relative offsets are 32-bit").  Its
left-hand side is 80 b * ((RA + 257) * sA + (RB + 1) * sB) for b-byte voxels; with the major axis x or y, sB = bnx * bny and sA = bnx
or 1.  RA x RB is the tile's own brick rectangle, found per tile and frame, not a constant of the kernel instance: RA <= 255, and
RB <= min(255, bnz), the bricks along z.  The volume holds 64 b * bnx * bny * bnz bytes, so where the second term reaches 2^31 the
volume has at least 0.8 * 2^31 * RB / (RB + 1) bytes: 0.86 GB with one brick of z (RB = 1, and then no offset comes near 2^31 on
either side: the large term is only ever added for tb >= 1), 1.7 GB where RB is large enough for offsets near 2^31 -- and there a
tile must be one brick wide and 150 to 255 bricks deep to be staged at all (3 * RA * RB slots have to fit its ring).  The first term
helps a little: with nx = 32768 and RA = 255 it is 0.67 GB (16-bit voxels, major axis x), and the limit is then crossed by a volume
of 0.6 GB.  Volumes of around 100 MiB lie far below the limit, whatever their shape.
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
O = _load("offset_limits", _HERE / "offset_limits.py")

GENERIC, FAST, RELAY, TSLAB = "raymarch_generic_kernel", "raymarch_fast_kernel", "raymarch_relay_kernel", "raymarch_tslab_kernel"
ISO, RESLICE, SHADE = "raymarch_iso_kernel", "reslice_kernel", "raymarch_shade_kernel"
SIZE = (96, 64)
ALPHA = 0.001                                       # low enough for the rays to cross the volume: 3000 samples stay below dest.a = 0.95
# windows no wider than 1024 values, so the fast kernel's 64-bit instances keep their address tables beside the cut classification table
WINDOW = {1: (10, 200), 2: (1500, 2500)}
COEF = E.COEFS[0]
DTYPES = pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
SIDES = pytest.mark.parametrize("side", ["inside", "outside"], ids=["32bit", "64bit"])
FILTERS = pytest.mark.parametrize("filt", [0, 1], ids=["nearest", "trilinear"])


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    d = tmp_path_factory.mktemp("offset_limits_refs")
    return {"iso": iso_ref.build(d), "shade": shade_ref.build(d), "reslice": reslice_ref.build(d)}


@pytest.fixture
def handle(vra):
    r = vra.RendererCore(0)
    yield r
    r.close()


_volumes = {}


def threshold_volume(dims, dtype, clear=True):
    """random voxels, with the quarter next to voxel (0, 0, 0) cleared for the kernels that skip; the last one drawn is kept for
    the next test"""
    key = (dims, np.dtype(dtype).name)
    if key not in _volumes:
        _volumes.clear()
        rng = np.random.default_rng(sum(dims) + np.dtype(dtype).itemsize)
        vol = O.rand_voxels(rng, dims, dtype)
        _volumes[key] = O.clear_first_corner(vol) if clear else vol
    return _volumes[key]


def same(got, want, what):
    problem = E.differ(got, want)
    assert not problem, f"{what}: {problem}"


def load(r, size, vol, spacing, layout):
    r.setup(size)
    assert r.loadShader("VolumeRenderer.cs")
    r.setQuirks(0)
    r.setLayout(layout)
    r.setVolume(vol, spacing)


def reads_the_last_voxel(render_ref, vol):
    """the reference's frame with the last voxel at its largest and at its smallest value: they differ when a sample of the frame
    reads voxel (nx - 1, ny - 1, nz - 1) -- a ray that has passed the last plane along every axis, where every factor of the
    address is largest.  The volume is restored."""
    keep = vol.flat[-1]
    frames = []
    for value in (E.vmax_of(vol.dtype), 0):
        vol.flat[-1] = value
        frames.append(render_ref())
    vol.flat[-1] = keep
    return bool(E.differ(frames[0], frames[1]))


def cameras(oracle, t, dims):
    """(view, name, block): the camera at the last voxel in the default view and from the top, and an orbit pose that shows the box"""
    c = oracle.Camera()
    c.orient(0.0, -0.3, 0.5)
    return [("front", "corner", O.corner_camera(E, dims, t.spacing, "front")), ("front", "orbit", c.block()),
            ("top", "corner", O.corner_camera(E, dims, t.spacing, "top"))]


# ---------------------------------------------------------------------------------------------------------------
# 1: both sides of every stride threshold
# ---------------------------------------------------------------------------------------------------------------
RAY_THRESHOLDS = pytest.mark.parametrize("name", [n for n, t in O.THRESHOLDS.items() if t.rays])


@RAY_THRESHOLDS
@SIDES
@DTYPES
@FILTERS
def test_composite_and_mip_kernels_on_both_sides_of_a_threshold(vra, oracle, handle, name, side, dtype, filt):
    """Generic (variant 1), fast (2, 5), relay (3: the 32-bit side's headline mode) under NEAREST; generic, staged (6) and unstaged
    (7) under TRILINEAR in the bricked layout, generic and the automatic choice in the linear one.  Composite, MIP and a transfer
    function, skipping off and on (the cleared quarter of the volume is what it skips), three cameras.  The frame of each filter's
    corner camera reads the last voxel.  Variant 3 is the observable of the side: relay_selected() takes the relay kernel for the
    headline mode -- grey composite, default view, no active skip grid -- exactly when the offsets are 32-bit; the other modes of
    these volumes stay with the fast kernel on either side (nx + ny + nz > 3072: no address tables for the relay kernel)."""
    t = O.THRESHOLDS[name]
    dims = getattr(t, side)
    b = np.dtype(dtype).itemsize
    small = side == "inside"
    assert O.takes_32bit_path(dims, b, t.layout) == small
    vol = threshold_volume(dims, dtype)
    lo, hi = WINDOW[b]
    r = handle
    load(r, SIZE, vol, t.spacing, t.layout)
    r.setWindow(lo, hi); r.setAlpha(ALPHA); r.setFilter(filt)
    if filt == 0:
        variants = ((1, GENERIC), (2, FAST), (5, FAST), (3, None))
    elif t.layout == O.BRICKED:
        variants = ((1, GENERIC), (6, TSLAB), (7, TSLAB))
    else:
        variants = ((1, GENERIC), (0, GENERIC))
    relays = 0
    for view, cname, block in cameras(oracle, t, dims):
        r.setInitialCameraRotation(view == "top", False)
        r.setCameraBlock(block)
        for mode in ("grey", "mip", "tf"):
            r.setMIP(mode == "mip")
            r.setTransferFunction(E.TF_ISO, E.TF_RGBA) if mode == "tf" else r.setTransferFunction()
            lut = r.getTransferLut() if mode == "tf" else None
            p = oracle.OracleParams(SIZE[0], SIZE[1], cam=block, alpha_scale=ALPHA, voxel_size=t.spacing, min_val=lo, max_val=hi, is_mip=int(mode == "mip"),
                                    view_top=int(view == "top"), filter=filt, tf_rgba=lut, threads=8)
            want, want_total, want_spp = oracle.render(vol, p, want_spp=True)
            assert want_total > 0
            if cname == "corner" and mode == "grey":
                assert reads_the_last_voxel(lambda: oracle.render(vol, p, want_spp=True)[::2], vol), (name, side, view)
            for variant, kernel in variants:
                for skip in ((False,) if variant == 1 else (False, True)):
                    r.setKernelVariant(variant); r.setSkipEmpty(skip)
                    r.render()
                    got = r.readPixels()
                    total, spp = r.countSamples(per_pixel=True)
                    ran = r.last_kernel_name
                    what = f"{name} {side} {dims} {np.dtype(dtype).name} filter {filt} {view} {cname} {mode} variant {variant} skip {skip} via {ran}"
                    if variant == 3:
                        headline = mode == "grey" and view == "front" and not skip
                        assert ran == (RELAY if headline and small else FAST), what
                        relays += int(ran == RELAY)
                    else:
                        assert ran == kernel, what
                    assert r.pack12Bytes() == 0, what
                    assert total == want_total, what
                    same((got, spp), (want, want_spp), what)
    assert relays == (2 if small and filt == 0 else 0)


@RAY_THRESHOLDS
@SIDES
@DTYPES
def test_isosurface_reslice_and_shading_on_both_sides_of_a_threshold(vra, oracle, refs, handle, name, side, dtype):
    """the three kernels on csrc/vr_sampler.h, NEAREST and TRILINEAR: the isosurface (depth included) and the shaded composite at
    the corner camera of the default view and of the top view, skipping off and on, the top view through a transfer function;
    reslice planes through the first and the last voxel (a MIP slab and a single sample) and the last plane of every axis"""
    t = O.THRESHOLDS[name]
    dims = getattr(t, side)
    b = np.dtype(dtype).itemsize
    assert O.takes_32bit_path(dims, b, t.layout) == (side == "inside")
    vol = threshold_volume(dims, dtype)
    lo, hi = WINDOW[b]
    iso = (lo + hi) // 2
    rng = np.random.default_rng(20261300)
    r = handle
    load(r, SIZE, vol, t.spacing, t.layout)
    r.setWindow(lo, hi); r.setAlpha(0.3); r.setMIP(False)
    for filt in (0, 1):
        r.setFilter(filt)
        for view in ("front", "top"):
            block = O.corner_camera(E, dims, t.spacing, view)
            r.setInitialCameraRotation(view == "top", False)
            r.setCameraBlock(block)
            tf = view == "top"
            r.setTransferFunction(E.TF_ISO, E.TF_RGBA) if tf else r.setTransferFunction()
            lut = r.getTransferLut() if tf else None
            p = oracle.OracleParams(SIZE[0], SIZE[1], cam=block, alpha_scale=0.3, voxel_size=t.spacing, min_val=lo, max_val=hi, view_top=int(view == "top"),
                                    filter=filt, tf_rgba=lut)
            want_iso = iso_ref.render(refs["iso"], vol, p, iso, u16_offset=False)
            want_shade = shade_ref.render(refs["shade"], vol, p, *COEF)
            assert np.isfinite(want_iso[1]).any() and want_shade[1].any()
            if not tf:
                assert reads_the_last_voxel(lambda: iso_ref.render(refs["iso"], vol, p, iso, u16_offset=False), vol), (name, side, filt, "iso")
                assert reads_the_last_voxel(lambda: shade_ref.render(refs["shade"], vol, p, *COEF), vol), (name, side, filt, "shade")
            for skip in (False, True):
                what = f"{name} {side} {dims} {np.dtype(dtype).name} filter {filt} {view} skip {skip}"
                r.setSkipEmpty(skip)
                r.setIsosurface(True, iso)
                r.render()
                assert r.last_kernel_name == ISO, what
                same((r.readPixels(), r.readDepth(), r.countSamples(per_pixel=True)[1]), want_iso, "iso " + what)
                r.setIsosurface(False)
                r.setShading(True, *COEF)
                r.render()
                assert r.last_kernel_name == SHADE, what
                same((r.readPixels(), r.countSamples(per_pixel=True)[1]), want_shade, "shade " + what)
                r.setShading(False)
        r.setInitialCameraRotation(False, False)
        r.setTransferFunction()
        r.setSkipEmpty(False)
        nx, ny, nz = dims
        planes = [("corners mip 3", E.corner_plane(rng, dims, SIZE, 3), "mip", 3), ("corners", E.corner_plane(rng, dims, SIZE, 1), "mean", 1)]
        for axis, n in enumerate(dims):                       # the last plane of every axis, around the last voxel
            o = np.array([nx - 70.0, ny - 50.0, nz - 50.0]); du = np.array([1.0, 0.0, 0.0]); dv = np.array([0.0, 1.0, 0.0]); dw = np.zeros(3)
            if axis == 0:
                o[0], du, dv = nx - 1.0, np.array([0.0, 1.0, 0.0]), np.array([0.0, 0.0, 1.0])
                o[1] = ny - 70.0
            elif axis == 1:
                o[1], dv = ny - 1.0, np.array([0.0, 0.0, 1.0])
            else:
                o[2] = nz - 1.0
            dw[axis] = 1.0
            planes.append((f"last plane of axis {axis}", np.concatenate([o, du, dv, dw]).astype(np.float32), "minip", 1))
        for pname, geom, red, n in planes:
            what = f"reslice {name} {side} {dims} {np.dtype(dtype).name} filter {filt} {pname}"
            want = reslice_ref.render(refs["reslice"], vol, geom, SIZE[0], SIZE[1], mode=red, n=n, filt=filt, min_val=lo, max_val=hi, u16_offset=False)
            assert want[2].any() and not want[2].all(), what       # pixels inside the volume and outside it
            r.setReslice(True, geom, mode=red, n=n)
            r.render()
            assert r.last_kernel_name == RESLICE, what
            same((r.readPixels(), r.readResliceValues(), r.countSamples(per_pixel=True)[1]), want, what)
            r.setReslice(False)


LINE_THRESHOLDS = pytest.mark.parametrize("name", [n for n, t in O.THRESHOLDS.items() if not t.rays])


def line_planes(dims):
    """64 x 48 planes of a long line of voxels: 64 consecutive x positions a row, rows a twelfth of a voxel apart in y and z from
    below the volume to above it.  The windows of x hold the first voxel, the last voxel (each with positions outside the volume
    beside it), the middle, and -- where the line is that long -- both sides of 2^23 and of 2^24 - 1."""
    nx, ny, nz = dims
    starts = {"first": -5, "last": nx - 59, "middle": nx // 2 - 32}
    if nx > (1 << 23) + 64:
        starts["2^23"] = (1 << 23) - 32
    if nx >= (1 << 24) - 1:
        starts["2^24 - 1"] = (1 << 24) - 1 - 50
    out = []
    for label, x0 in starts.items():
        o = np.array([x0, -0.75, -0.75])
        dv = np.array([0.0, (ny + 0.5) / 48.0, (nz + 0.5) / 48.0])
        out.append((label, np.concatenate([o, [1.0, 0.0, 0.0], dv, [0.0, 0.0, 1.0]]).astype(np.float32)))
    return out


@LINE_THRESHOLDS
@SIDES
@DTYPES
def test_reslice_along_lines_of_voxels_on_both_sides_of_a_threshold(vra, oracle, refs, handle, name, side, dtype):
    """2^20 x 4 x 4 (bricked: bstride_y) and 2^24 - 1 voxels in a row (linear: a dimension) and their neighbours on the 64-bit
    side: no camera ray crosses them usefully within 10 000 steps, so they are read through reslice planes, NEAREST and TRILINEAR,
    values included.  vr_set_volume takes 2^24 voxels along one axis (the 64-bit side of `dimension` runs)."""
    t = O.THRESHOLDS[name]
    dims = getattr(t, side)
    b = np.dtype(dtype).itemsize
    assert O.takes_32bit_path(dims, b, t.layout) == (side == "inside")
    vol = threshold_volume(dims, dtype, clear=False)
    lo, hi = WINDOW[b]
    size = (64, 48)
    r = handle
    load(r, size, vol, t.spacing, t.layout)
    r.setWindow(lo, hi)
    for filt in (0, 1):
        r.setFilter(filt)
        for label, geom in line_planes(dims):
            for red, n in (("mip", 1), ("mean", 2)):
                what = f"reslice {name} {side} {dims} {np.dtype(dtype).name} filter {filt} x window {label} {red} n {n}"
                want = reslice_ref.render(refs["reslice"], vol, geom, size[0], size[1], mode=red, n=n, filt=filt, min_val=lo, max_val=hi, u16_offset=False)
                assert want[2].any() and not want[2].all(), what
                r.setReslice(True, geom, mode=red, n=n)
                r.render()
                assert r.last_kernel_name == RESLICE, what
                same((r.readPixels(), r.readResliceValues(), r.countSamples(per_pixel=True)[1]), want, what)
                r.setReslice(False)
    _volumes.clear()


# ---------------------------------------------------------------------------------------------------------------
# 2: the 32-bit path with bit 31 of the offset set
# ---------------------------------------------------------------------------------------------------------------
BIG_SIZE = (64, 48)
BIG_WINDOW = {1: (1, 64), 2: (16, 1024)}            # the thin noise of the outer planes carries weight; the ball's core saturates
BIG_ALPHA = 0.0005                                  # no ray reaches dest.a >= 0.95: all of them cross the whole volume
BIG_ROWS = (20, 28)                                 # the rows of the isosurface and shading frames (the references' time)


@pytest.fixture(scope="module", params=list(O.BIG_VOLUMES))
def big(vra, request):
    """one handle per volume: generated on the device in the volume's first layout, read back once"""
    R = vra.renderer
    v = O.BIG_VOLUMES[request.param]
    r = vra.RendererCore(0)
    r.setup(BIG_SIZE)
    assert r.loadShader("VolumeRenderer.cs")
    r.setQuirks(0)
    r.setLayout(v.layouts[0])
    r.generateSynthetic(R.SYNTH_NOISE_BALL, v.dims, v.bytes_per_voxel, 0x9E3779B9 ^ sum(v.dims))
    vol = r.readVolume()
    assert vol.shape == v.dims[::-1] and vol.dtype.itemsize == v.bytes_per_voxel
    r.setWindow(*BIG_WINDOW[v.bytes_per_voxel])
    yield v, r, vol
    r.close()


def big_planes(v, layout, filt):
    """(name, geometry, reduction, n, exact): axial planes over the whole xy extent at whole-voxel strides -- the last plane, the
    first one with an offset of 2^31 bytes (16-bit) or elements (8-bit) and the one before it; under TRILINEAR a quarter of a
    voxel off the grid, so the lerps mix the planes on either side -- and an oblique slab that rises through the last brick layer
    and leaves the volume.  exact: NEAREST at voxel centres, the values are the host array's."""
    nx, ny, nz = v.dims
    sx, sy = nx // 64, ny // 48
    x0, y0 = nx - 1 - 63 * sx, ny - 1 - 47 * sy
    first = O.first_plane_with_bit31(v.dims, v.bytes_per_voxel, layout)
    off = 0.0 if filt == 0 else 0.25
    out = []
    for name, k in (("last plane", nz - 1), ("first plane with bit 31", first), ("the plane before it", first - 1)):
        geom = [x0 - off, y0 - off, k - off, sx, 0, 0, 0, sy, 0, 0, 0, 1]
        out.append((f"{name} (k = {k})", np.array(geom, dtype=np.float32), "mip", 1, filt == 0))
    geom = [0, 0, nz - 4.5, nx / 64.0, 0, 0.03, 0, ny / 48.0, 0.04, 0, 0, 0.5]
    out.append(("oblique slab through the last brick layer", np.array(geom, dtype=np.float32), "mean", 3, False))
    return out


@FILTERS
def test_reslice_reads_the_voxels_whose_offsets_have_bit_31_set(vra, refs, big, filt):
    v, r, vol = big
    b = v.bytes_per_voxel
    assert sum(v.dims) > 3072
    lo, hi = BIG_WINDOW[b]
    nx, ny, nz = v.dims
    r.setFilter(filt)
    try:
        for layout in v.layouts:
            assert O.takes_32bit_path(v.dims, b, layout)
            r.setLayout(layout)
            for name, geom, red, n, exact in big_planes(v, layout, filt):
                what = f"{v.name} layout {layout} filter {filt} {name}"
                want = reslice_ref.render(refs["reslice"], vol, geom, BIG_SIZE[0], BIG_SIZE[1], mode=red, n=n, filt=filt, min_val=lo, max_val=hi, u16_offset=False)
                r.setReslice(True, geom, mode=red, n=n)
                r.render()
                assert r.last_kernel_name == RESLICE, what
                got = (r.readPixels(), r.readResliceValues(), r.countSamples(per_pixel=True)[1])
                same(got, want, what)
                if exact:
                    k = int(geom[2])
                    host = vol[k, int(geom[1])::int(geom[7]), int(geom[0])::int(geom[3])].astype(np.float32)
                    assert host.shape == got[1].shape and np.array_equal(got[1], host), what
                    assert len(np.unique(host)) > 8, what                 # a plane of noise, not of one value
                else:
                    assert want[2].any(), what
    finally:
        r.setReslice(False); r.setFilter(0); r.setLayout(v.layouts[0])


@pytest.mark.parametrize("view", ["front", "top"])
def test_ray_marched_modes_cross_the_voxels_whose_offsets_have_bit_31_set(vra, oracle, refs, big, view):
    """whole 64 x 48 frames at an opacity at which every ray crosses the whole volume: generic and fast composite, MIP, a transfer
    function with skipping (NEAREST); generic, unstaged and staged TRILINEAR (the latter two in the bricked layout); eight rows of
    the isosurface with its depth and of the shaded composite.  nx + ny + nz > 3072: no packed copy, no batched TRILINEAR kernel."""
    v, r, vol = big
    b = v.bytes_per_voxel
    lo, hi = BIG_WINDOW[b]
    w, h = BIG_SIZE
    top = view == "top"
    try:
        r.setInitialCameraRotation(top, False)
        r.resetCamera()
        r.cameraOrient(0.0, 0.06 * 3, 0.06 * 5)          # a little off the axis: the rays cross brick columns
        block = r.getCameraBlock()
        r.setAlpha(BIG_ALPHA)
        frames = {}

        def reference(mode, filt, lut):
            key = (mode, filt)
            if key not in frames:
                p = oracle.OracleParams(w, h, cam=block, alpha_scale=BIG_ALPHA, min_val=lo, max_val=hi, is_mip=int(mode == "mip"), view_top=int(top),
                                        filter=filt, tf_rgba=lut, threads=8)
                frames[key] = oracle.render(vol, p, want_spp=True)
                assert frames[key][1] > 0
            return frames[key]

        for layout in v.layouts:
            r.setLayout(layout)
            cases = [("grey", 0, 1, False, GENERIC), ("grey", 0, 2, False, FAST), ("grey", 0, 5, False, FAST), ("mip", 0, 2, False, FAST),
                     ("tf", 0, 2, True, FAST), ("grey", 1, 1, False, GENERIC)]
            if layout == O.BRICKED:
                cases += [("grey", 1, 7, False, TSLAB), ("grey", 1, 6, False, TSLAB), ("tf", 1, 6, True, TSLAB)]
            for mode, filt, variant, skip, kernel in cases:
                r.setFilter(filt); r.setMIP(mode == "mip"); r.setKernelVariant(variant); r.setSkipEmpty(skip)
                r.setTransferFunction(E.TF_ISO, E.TF_RGBA) if mode == "tf" else r.setTransferFunction()
                lut = r.getTransferLut() if mode == "tf" else None
                want, want_total, want_spp = reference(mode, filt, lut)
                r.render()
                what = f"{v.name} layout {layout} {view} {mode} filter {filt} variant {variant} skip {skip} via {r.last_kernel_name}"
                assert r.last_kernel_name == kernel, what
                assert r.pack12Bytes() == 0, what
                got = r.readPixels()
                total, spp = r.countSamples(per_pixel=True)
                assert total == want_total, what
                same((got, spp), (want, want_spp), what)
            # the isosurface and the shaded composite, eight rows
            r.setKernelVariant(0); r.setMIP(False); r.setTransferFunction()
            r.setRowRange(*BIG_ROWS)
            rows = slice(*BIG_ROWS)
            iso = (lo + hi) // 2
            for filt in (0, 1):
                r.setFilter(filt)
                p = oracle.OracleParams(w, h, cam=block, alpha_scale=BIG_ALPHA, min_val=lo, max_val=hi, view_top=int(top), filter=filt,
                                        row_begin=BIG_ROWS[0], row_end=BIG_ROWS[1])
                key = ("iso+shade", filt)
                if key not in frames:
                    frames[key] = (iso_ref.render(refs["iso"], vol, p, iso, u16_offset=False), shade_ref.render(refs["shade"], vol, p, *COEF))
                want_iso, want_shade = frames[key]
                assert np.isfinite(want_iso[1][rows]).any() and want_shade[1][rows].any()
                for skip in (False, True):
                    what = f"{v.name} layout {layout} {view} filter {filt} skip {skip}"
                    r.setSkipEmpty(skip)
                    r.setIsosurface(True, iso)
                    r.render()
                    assert r.last_kernel_name == ISO, what
                    got = (r.readPixels(), r.readDepth(), r.countSamples(per_pixel=True)[1])
                    same([a[rows] for a in got], [a[rows] for a in want_iso], "iso " + what)
                    r.setIsosurface(False)
                    r.setShading(True, *COEF)
                    r.render()
                    assert r.last_kernel_name == SHADE, what
                    got = (r.readPixels(), r.countSamples(per_pixel=True)[1])
                    same([a[rows] for a in got], [a[rows] for a in want_shade], "shade " + what)
                    r.setShading(False)
            r.setRowRange(0, -1)
    finally:
        r.setRowRange(0, -1); r.setIsosurface(False); r.setShading(False); r.setSkipEmpty(False); r.setKernelVariant(0); r.setFilter(0)
        r.setMIP(False); r.setTransferFunction(); r.setInitialCameraRotation(False, False); r.resetCamera(); r.setLayout(v.layouts[0])
