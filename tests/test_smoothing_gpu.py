"""vr_smooth_volume on the device against its CPU definition (tests/smooth_ref/smooth_ref.c), bit for bit: the voxels read back
over both voxel types, both layouts, shapes that are no multiple of a brick or a tile and axes shorter than the radius; that
smoothing never accumulates and (0, 0, 0) restores the loaded volume and every mode's frame; that everything built from the
voxels (packed copy, apron copies, skip grid, ranges, tile order) follows them, by comparing with a fresh handle that was
given the CPU-smoothed voxels; what the call keeps; layout changes; and a volume beyond 32-bit byte offsets on sampled voxels.
The kernels at the limits of their LDS ring, column segments, x tiles and z slabs: tests/test_smoothing_edges_gpu.py."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("smooth_ref_binding", Path(__file__).resolve().parent / "smooth_ref" / "binding.py")
smooth_ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(smooth_ref)

SIGMAS = [(1.0, 1.0, 1.0), (0.5, 2.0, 0.0), (0.0, 0.0, 3.0), (8.0, 0.3, 1.0)]
SHAPES = [(13, 11, 6), (70, 66, 68), (5, 3, 1), (64, 1, 1)]          # (nx, ny, nz)
TF_ISO = [0, 60, 140, 255]
TF_RGBA = [[0.2, 0.9, 0.1, 0.0], [0.9, 0.3, 0.2, 0.4], [1.0, 0.8, 0.6, 0.8], [0.5, 0.5, 1.0, 1.0]]


@pytest.fixture(scope="module")
def smoothlib(tmp_path_factory):
    return smooth_ref.build(tmp_path_factory.mktemp("smooth_ref_gpu"))


@pytest.fixture(scope="module")
def handles(vra):
    """two renderers with a 64 x 48 target: the one under test and the fresh one it is compared with"""
    hs = []
    for _ in range(2):
        r = vra.RendererCore(0)
        r.setup((64, 48))
        assert r.loadShader("VolumeRenderer.cs")
        hs.append(r)
    yield hs
    for r in hs:
        r.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def weights_for(vra, sigmas):
    return tuple(vra.smooth_weights(s) if s > 0 else None for s in sigmas)


_REF = {}


def reference(vra, smoothlib, key, vol, sig):
    """the CPU definition's result, computed once per (volume key, sigmas) and shared"""
    k = (key, tuple(sig))
    if k not in _REF:
        out = smooth_ref.smooth(smoothlib, vol, weights_for(vra, sig))
        out.setflags(write=False)
        _REF[k] = out
    return _REF[k]


def random_volume(shape_xyz, dtype, seed):
    nx, ny, nz = shape_xyz
    hi = 256 if dtype == np.uint8 else 65536
    return np.random.default_rng(seed).integers(0, hi, size=(nz, ny, nx)).astype(dtype)


def first_difference(got, want):
    bad = np.argwhere(got != want)
    z, y, x = bad[0]
    return f"{len(bad)} voxels differ, first (x {x}, y {y}, z {z}): {got[z, y, x]} vs {want[z, y, x]}"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_read_volume_after_smoothing_matches_the_reference(vra, smoothlib, handles, shape, dtype):
    r = handles[0]
    vol = random_volume(shape, dtype, 11)
    for layout in (vra.renderer.LAYOUT_LINEAR, vra.renderer.LAYOUT_BRICKED):
        r.setLayout(layout)
        r.setVolume(vol)
        for sig in SIGMAS:
            r.smoothVolume(sigma_voxels=sig)
            assert r.smoothing == tuple(float(np.float32(s)) for s in sig)
            got = r.readVolume()
            want = reference(vra, smoothlib, (shape, np.dtype(dtype).name, 11), vol, sig)
            assert np.array_equal(got, want), f"{shape} {np.dtype(dtype).name} layout {layout} sigma {sig}: " + first_difference(got, want)


@pytest.mark.parametrize("layout", [0, 1], ids=["linear", "bricked"])
def test_full_range_u16_with_the_extremes_at_the_corners(vra, smoothlib, handles, layout):
    r = handles[0]
    vol = random_volume((33, 32, 31), np.uint16, 12)
    vol[0, 0, 0] = 65535; vol[-1, -1, -1] = 0; vol[0, -1, 0] = 0; vol[-1, 0, -1] = 65535
    vol[0, 0, -1] = 65535; vol[0, 0, -2] = 65535; vol[0, 1, -1] = 65535; vol[1, 0, -1] = 65535      # a saturated corner block
    r.setLayout(layout)
    r.setVolume(vol)
    for sig in SIGMAS:
        r.smoothVolume(sigma_voxels=sig)
        got = r.readVolume()
        want = reference(vra, smoothlib, ("full16", 12), vol, sig)
        assert np.array_equal(got, want), f"layout {layout} sigma {sig}: " + first_difference(got, want)
    assert int(got.max()) <= 65535 and r.dataset_range[1] == int(want.max())


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_z_slabs_give_the_same_voxels_as_one_piece(vra, smoothlib, handles, dtype):
    """the fp32 planes bounded to a few planes of the 70 x 66 x 68 volume: several slabs, each with its halo planes"""
    r = handles[0]
    R = vra.renderer
    shape = (70, 66, 68)
    vol = random_volume(shape, dtype, 11)
    plane = 70 * 66 * 4
    r.setLayout(R.LAYOUT_BRICKED)
    r.setVolume(vol)
    try:
        for sig, planes in (((1.0, 1.0, 1.0), 11), ((0.0, 2.0, 3.0), 19), ((0.5, 2.0, 0.0), 5), ((8.0, 0.3, 1.0), 7)):
            r.setSmoothingWorkspace(planes * plane + 17)
            r.smoothVolume(sigma_voxels=sig)
            got = r.readVolume()
            want = reference(vra, smoothlib, (shape, np.dtype(dtype).name, 11), vol, sig)
            assert np.array_equal(got, want), f"{np.dtype(dtype).name} sigma {sig}, {planes} planes: " + first_difference(got, want)
        # a workspace below one slab (2 r_z + 1 planes) is an allocation failure: the handle keeps what it rendered
        r.setSmoothingWorkspace(6 * plane)
        with pytest.raises(vra.VRError) as e:
            r.smoothVolume(sigma_voxels=(1.0, 1.0, 1.0))
        assert e.value.code == R.VR_E_NOMEM
        assert r.smoothing == (8.0, float(np.float32(0.3)), 1.0) and np.array_equal(r.readVolume(), want)
    finally:
        r.setSmoothingWorkspace(0)


# ---------------------------------------------------------------- frames of every mode
MODES = ["composite", "mip", "trilinear", "iso", "shade", "reslice"]


def set_mode(vra, r, mode, dims):
    R = vra.renderer
    r.setIsosurface(False)
    r.setReslice(False)
    r.setShading(False)
    r.setMIP(mode == "mip")
    r.setFilter(R.FILTER_TRILINEAR if mode == "trilinear" else R.FILTER_NEAREST)
    if mode == "iso":
        r.setIsosurface(True, 120)
    elif mode == "shade":
        r.setShading(True, 0.2, 0.7, 0.3, 8)
    elif mode == "reslice":
        r.setReslice(True, vra.axis_reslice(2, dims[2] // 2, dims, (1.0, 1.0, 1.0), r.framebuffer_size, n=5), mode="mean", n=5)


def frame(r):
    r.render()
    rgba = r.readPixels().copy()
    total, spp = r.countSamples(per_pixel=True)
    return rgba, spp.copy(), total


def assert_same_frame(got, want, what):
    assert np.array_equal(bits(got[0]), bits(want[0])), f"{what}: {int(np.sum(bits(got[0]) != bits(want[0])))} floats of the frame differ"
    assert np.array_equal(got[1], want[1]) and got[2] == want[2], f"{what}: sample counts differ"


def test_smoothing_does_not_accumulate_and_zero_restores_the_loaded_volume(vra, oracle, smoothlib, handles):
    r = handles[0]
    R = vra.renderer
    dims = (41, 39, 40)
    vol = oracle.gen_noise_ball(dims, 1, 77)
    r.setLayout(R.LAYOUT_BRICKED)
    r.setVolume(vol)
    r.setWindow(20, 230)
    r.setAlpha(0.3)
    before = {}
    for m in MODES:
        set_mode(vra, r, m, dims)
        before[m] = frame(r)
    r.smoothVolume(sigma_voxels=(1.0, 1.0, 1.0))
    once = r.readVolume()
    assert np.array_equal(once, reference(vra, smoothlib, ("ball8", 77), vol, (1.0, 1.0, 1.0)))
    r.smoothVolume(sigma_voxels=(2.0, 2.0, 2.0))
    assert np.array_equal(r.readVolume(), reference(vra, smoothlib, ("ball8", 77), vol, (2.0, 2.0, 2.0)))
    set_mode(vra, r, "composite", dims)
    assert not np.array_equal(bits(frame(r)[0]), bits(before["composite"][0]))        # the frames do show the smoothed volume
    r.smoothVolume(sigma_voxels=0.0)
    assert r.smoothing == (0.0, 0.0, 0.0)
    assert np.array_equal(r.readVolume(), vol)
    for m in MODES:
        set_mode(vra, r, m, dims)
        assert_same_frame(frame(r), before[m], f"{m} after (0, 0, 0)")
    set_mode(vra, r, "composite", dims)


def configure(vra, r, case, dims):
    R = vra.renderer
    set_mode(vra, r, "composite", dims)
    r.setKernelVariant(0)
    r.setSkipEmpty(False)
    r.setTransferFunction()
    r.setAlpha(0.3)
    if case == "nearest_tf_skip":
        r.setTransferFunction(TF_ISO, TF_RGBA)
        r.setSkipEmpty(True)
    elif case == "trilinear_staged":
        r.setFilter(R.FILTER_TRILINEAR)
        r.setKernelVariant(6)
        r.setSkipEmpty(True)
    elif case == "iso_skip":
        set_mode(vra, r, "iso", dims)
        r.setSkipEmpty(True)
    elif case == "shade":
        set_mode(vra, r, "shade", dims)
        r.setTransferFunction(TF_ISO, TF_RGBA)
        r.setSkipEmpty(True)
    elif case == "reslice":
        set_mode(vra, r, "reslice", dims)


CASES = ["nearest_pack12", "nearest_tf_skip", "trilinear_staged", "iso_skip", "shade", "reslice"]


@pytest.mark.parametrize("case", CASES)
def test_everything_derived_from_the_voxels_follows_the_smoothing(vra, smoothlib, handles, case):
    """a handle that rendered the loaded volume (so every copy, grid and order of it exists), then smoothed it, against a fresh
    handle that was given the CPU-smoothed voxels and the same window"""
    r, f = handles
    R = vra.renderer
    dims = (41, 39, 40)
    rng = np.random.default_rng(21)
    sig = (1.0, 1.5, 1.0)
    # 16-bit data inside a ball, zero outside: empty cells for the skip grid, and its shell moves when the data are smoothed
    zz, yy, xx = np.meshgrid(np.arange(40), np.arange(39), np.arange(41), indexing="ij")
    ball = (xx - 20) ** 2 + (yy - 19) ** 2 + (zz - 20) ** 2 < 15 ** 2
    vol = np.where(ball, rng.integers(1000, 3000, size=ball.shape), 0).astype(np.uint16)
    window = (-1000, 3095)                                    # stored 0 .. 4095 under VR_QUIRK_U16_OFFSET: a divisor the fast kernels are certified for
    for r_ in (r, f):
        r_.setLayout(R.LAYOUT_BRICKED)
        configure(vra, r_, case, dims)
    if case == "nearest_pack12":
        # spikes: the loaded range (0 .. 20000) rules the packed copy out, the smoothed one (within 4096 values) allows it
        spikes = vol.copy()
        spikes[5::9, 4::9, 3::9] = 20000
        want = reference(vra, smoothlib, ("spikes", 21), spikes, sig)
        assert int(want.max()) - int(want.min()) <= 4095
        r.setVolume(spikes)
        r.setWindow(*window)
        loaded = frame(r)
        assert r.pack12Bytes() == 0
        r.smoothVolume(sigma_voxels=sig)
        f.setVolume(want)
        f.setWindow(*window)
        assert_same_frame(frame(r), frame(f), "packed copy after smoothing")
        assert r.pack12Bytes() == f.pack12Bytes() > 0
        assert r.dataset_range == f.dataset_range and np.array_equal(r.histogram(), f.histogram())
        # the converse: back on the loaded volume the copy of the smoothed one must not be used again
        r.smoothVolume(sigma_voxels=0.0)
        assert_same_frame(frame(r), loaded, "loaded volume after (0, 0, 0)")
        assert r.pack12Bytes() == 0
        # ... and a copy built from the loaded voxels (minimum 0 folded into it) is rebuilt from the smoothed ones
    want = reference(vra, smoothlib, ("ball16", 21), vol, sig)
    r.setVolume(vol)
    r.setWindow(*window)
    stale = frame(r)
    if case == "nearest_pack12":
        assert r.pack12Bytes() > 0
    if case == "trilinear_staged":
        assert r.last_kernel_name == "raymarch_tslab_kernel"
    r.takeMessage()
    r.smoothVolume(sigma_voxels=sig)
    assert r.window == window and r.takeMessage() is None
    f.setVolume(want)
    f.setWindow(*window)
    got, fresh = frame(r), frame(f)
    assert_same_frame(got, fresh, case)
    assert not np.array_equal(bits(got[0]), bits(stale[0]))
    assert r.pack12Bytes() == f.pack12Bytes()
    assert r.dataset_range == f.dataset_range
    assert np.array_equal(r.histogram(), f.histogram())
    assert np.array_equal(r.readVolume(), want)
    for r_ in (r, f):
        configure(vra, r_, "nearest_pack12", dims)


def test_the_call_keeps_the_users_state_and_queues_no_message(vra, oracle, handles):
    r = handles[0]
    R = vra.renderer
    vol = oracle.gen_noise_ball((24, 20, 22), 2, 5)
    r.setLayout(R.LAYOUT_BRICKED)
    r.setVolume(vol, (0.5, 1.0, 2.0))
    r.setWindow(-300, 2500)
    r.cameraOrient(1.0, 0.4, -0.7)
    r.setFilter(R.FILTER_TRILINEAR)
    r.setShading(True, 0.25, 0.5, 0.125, 64)
    r.setTransferFunction(TF_ISO, TF_RGBA)
    r.setMIP(True)
    r.takeMessage()
    cam, lut, shading, dims = r.getCameraBlock(), r.getTransferLut(), r.shading(), r.dims
    mip = frame(r)
    r.smoothVolume(sigma_mm=(1.0, 1.0, 1.0))
    assert r.smoothing == (2.0, 1.0, 0.5)                       # millimetres over the spacing, per axis
    assert r.takeMessage() is None
    assert r.window == (-300, 2500)
    assert np.array_equal(bits(r.getCameraBlock()), bits(cam))
    assert np.array_equal(bits(r.getTransferLut()), bits(lut))
    assert r.shading() == shading and r.dims == dims
    assert not np.array_equal(bits(frame(r)[0]), bits(mip[0]))  # still MIP with TRILINEAR, now of the smoothed volume
    assert r.last_kernel_name != "raymarch_shade_kernel"
    r.smoothVolume(sigma_voxels=0.0)
    assert_same_frame(frame(r), mip, "the MIP frame after (0, 0, 0)")
    r.setMIP(False); r.setShading(False); r.setTransferFunction(); r.setFilter(R.FILTER_NEAREST); r.resetCamera()


def test_set_layout_after_smoothing_relays_both_volumes(vra, smoothlib, handles):
    r = handles[0]
    R = vra.renderer
    dims = (41, 39, 40)
    vol = random_volume(dims, np.uint8, 31)
    sig = (1.0, 0.5, 2.0)
    want = reference(vra, smoothlib, ("layout8", 31), vol, sig)
    for first, second in ((R.LAYOUT_BRICKED, R.LAYOUT_LINEAR), (R.LAYOUT_LINEAR, R.LAYOUT_BRICKED)):
        r.setLayout(first)
        r.setVolume(vol)
        r.setWindow(10, 240)
        r.setKernelVariant(1)                                # the generic kernel renders both layouts: the frames must be the same bits
        loaded = frame(r)
        r.smoothVolume(sigma_voxels=sig)
        smoothed = frame(r)
        r.setLayout(second)
        assert r.smoothing == tuple(float(np.float32(s)) for s in sig)
        assert np.array_equal(r.readVolume(), want)
        assert_same_frame(frame(r), smoothed, f"layout {first} -> {second}")
        r.smoothVolume(sigma_voxels=0.0)
        assert np.array_equal(r.readVolume(), vol)
        assert_same_frame(frame(r), loaded, f"(0, 0, 0) after layout {first} -> {second}")
    r.setKernelVariant(0)
    r.setLayout(R.LAYOUT_BRICKED)


def test_loading_resets_the_state_and_the_kept_volume_is_counted_under_other(vra, oracle, handles):
    r = handles[0]
    R = vra.renderer
    r.setLayout(R.LAYOUT_BRICKED)
    vol = oracle.gen_noise_ball((40, 40, 40), 2, 9)
    r.setVolume(vol)
    v0, c0, o0 = r.residentBytes()
    r.smoothVolume(sigma_voxels=(1.0, 0.0, 2.0))
    v1, c1, o1 = r.residentBytes()
    assert v1 == v0 and o1 == o0 + v0 and c1 == 0              # the rendered volume; the kept loaded one under `other`, never a copy
    r.setCopyBudget(0)
    assert r.residentBytes() == (v0, 0, o0 + v0)
    r.setCopyBudget(r.COPY_BUDGET_AUTO)
    r.smoothVolume(sigma_voxels=0.0)
    assert r.residentBytes() == (v0, 0, o0)
    r.smoothVolume(sigma_voxels=(1.0, 0.0, 2.0))
    r.setVolume(vol)
    assert r.smoothing == (0.0, 0.0, 0.0) and r.residentBytes()[2] == o0
    r.smoothVolume(sigma_voxels=(1.0, 0.0, 2.0))
    r.generateSynthetic(R.SYNTH_NOISE_BALL, (32, 32, 32), 1, 3)
    assert r.smoothing == (0.0, 0.0, 0.0)
    r.smoothVolume(sigma_voxels=0.0)                           # nothing to drop: a no-op
    assert r.smoothing == (0.0, 0.0, 0.0)


def test_errors_change_nothing(vra, oracle, handles):
    R = vra.renderer
    fresh = vra.RendererCore(0)
    try:
        fresh.setup((64, 48))
        assert fresh.loadShader("VolumeRenderer.cs")
        with pytest.raises(vra.VRError) as e:
            fresh.smoothVolume(sigma_voxels=(1.0, 1.0, 1.0))   # before any volume: what vr_read_volume gives
        assert e.value.code == R.VR_E_INVALID
        assert fresh.smoothing == (0.0, 0.0, 0.0)
    finally:
        fresh.close()
    r = handles[0]
    vol = oracle.gen_noise_ball((24, 20, 22), 1, 5)
    r.setLayout(R.LAYOUT_BRICKED)
    r.setVolume(vol)
    r.setWindow(10, 240)
    r.smoothVolume(sigma_voxels=(1.0, 2.0, 0.5))
    voxels, fr = r.readVolume(), frame(r)
    for bad in ((-1.0, 1.0, 1.0), (1.0, float("nan"), 1.0), (1.0, 1.0, 8.25), (float("inf"), 0.0, 0.0), (0.0, 0.0, -0.0001)):
        with pytest.raises(vra.VRError) as e:
            r.smoothVolume(sigma_voxels=bad)
        assert e.value.code == R.VR_E_INVALID, bad
        assert r.smoothing == (1.0, 2.0, 0.5)
    assert np.array_equal(r.readVolume(), voxels)
    assert_same_frame(frame(r), fr, "after refused calls")
    r.smoothVolume(sigma_voxels=0.0)


def test_beyond_32_bit_offsets_on_sampled_voxels(vra, smoothlib):
    """2048 x 2048 x 520 u16, bricked: 4.06 GiB of voxels; the storage offset 2^32 bytes is the first voxel of brick layer 128,
    (0, 0, 512).  The fp32 planes of this volume do not fit the automatic workspace in one piece, so the call also runs in z
    slabs.  About 2000 voxels against the pointwise CPU definition: the first and the last voxel, both sides of the 2^32-byte
    offset, slab seams, random ones.  (z is already the smallest multiple of 8 that leaves a brick layer beyond the offset's.)"""
    R = vra.renderer
    nx, ny, nz = 2048, 2048, 520
    r = vra.RendererCore(0)
    try:
        r.setup((64, 48))
        assert r.loadShader("VolumeRenderer.cs")
        r.setLayout(R.LAYOUT_BRICKED)
        r.generateSynthetic(R.SYNTH_NOISE_BALL, (nx, ny, nz), 2, 0xBEEF)
        vol = r.readVolume()
        sig = (0.5, 0.5, 0.5)
        r.smoothVolume(sigma_voxels=sig)
        got = r.readVolume()
        rng = np.random.default_rng(32)
        pts = [(0, 0, 0), (nx - 1, ny - 1, nz - 1), (0, 0, 511), (3, 3, 511), (nx - 1, ny - 1, 511), (0, 0, 512), (1, 0, 512), (0, 1, 512),
               (nx - 1, ny - 1, 512), (0, 0, 513), (nx - 1, 0, 0), (0, ny - 1, nz - 1)]
        for z in (509, 510, 511, 512, 513, 514):
            pts += [(int(x), int(y), z) for x, y in rng.integers(0, 2048, size=(60, 2))]
        for z in range(120, 132):                             # around the first slab seam of a 2 GiB workspace (128 planes, 124 outputs)
            pts += [(int(x), int(y), z) for x, y in rng.integers(0, 2048, size=(20, 2))]
        pts += [(int(x), int(y), int(z)) for x, y, z in zip(rng.integers(0, nx, 1400), rng.integers(0, ny, 1400), rng.integers(0, nz, 1400))]
        ijk = np.asarray(pts, dtype=np.int32)
        want = smooth_ref.smooth_points(smoothlib, vol, weights_for(vra, sig), ijk)
        have = got[ijk[:, 2], ijk[:, 1], ijk[:, 0]]
        bad = np.flatnonzero(have != want)
        assert bad.size == 0, f"{bad.size} of {len(pts)} sampled voxels differ, first {tuple(ijk[bad[0]])}: {have[bad[0]]} vs {want[bad[0]]}"
        assert np.any(have != vol[ijk[:, 2], ijk[:, 1], ijk[:, 0]])                  # the samples do see the smoothing
    finally:
        r.close()
