"""vr_rank_filter_volume on the device against its brute-force CPU definition (tests/rank_ref/rank_ref.c), bit for bit: the
voxels read back over both voxel types, both layouts, shapes that are no multiple of a brick or a tile and axes shorter than
the radius; values either side of the sign bit; medians of volumes with two and three distinct values; the column kernels at
the limits of their LDS ring and segments and the tiles' seams (tests/rank_filter_cases.py); the state a call keeps, drops and
resets; its composition with vr_smooth_volume; everything derived from the voxels, against a fresh handle that was given the
CPU-filtered voxels; and a volume beyond 32-bit offsets on sampled voxels."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = Path(__file__).resolve().parent


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


cases = _load("rank_filter_cases", HERE / "rank_filter_cases.py")
rank_ref = _load("rank_ref_binding", HERE / "rank_ref" / "binding.py")
smooth_ref = _load("smooth_ref_binding", HERE / "smooth_ref" / "binding.py")

OFF, ERODE, DILATE, OPEN, CLOSE, MEDIAN = range(6)
TF_ISO = [0, 60, 140, 255]
TF_RGBA = [[0.2, 0.9, 0.1, 0.0], [0.9, 0.3, 0.2, 0.4], [1.0, 0.8, 0.6, 0.8], [0.5, 0.5, 1.0, 1.0]]


@pytest.fixture(scope="module")
def ranklib(tmp_path_factory):
    return rank_ref.build(tmp_path_factory.mktemp("rank_ref_gpu"))


@pytest.fixture(scope="module")
def smoothlib(tmp_path_factory):
    return smooth_ref.build(tmp_path_factory.mktemp("rank_smooth_ref_gpu"))


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


_REF = {}


def reference(ranklib, key, vol, op, radius):
    """the CPU definition's result, computed once per (volume key, op, radii) and shared"""
    radius = tuple(int(v) for v in np.broadcast_to(np.asarray(radius), (3,)))
    k = (key, op, radius)
    if k not in _REF:
        out = rank_ref.rank(ranklib, vol, op, radius)
        out.setflags(write=False)
        _REF[k] = out
    return _REF[k]


def first_difference(got, want):
    bad = np.argwhere(got != want)
    z, y, x = bad[0]
    return f"{len(bad)} voxels differ, first (x {x}, y {y}, z {z}): {got[z, y, x]} vs {want[z, y, x]}"


def check_voxels(r, ranklib, key, vol, op, radius, what):
    r.rankFilterVolume(op, radius)
    got = r.readVolume()
    want = reference(ranklib, key, vol, op, radius)
    assert np.array_equal(got, want), f"{what} {cases.OP_NAMES[op]} {radius}: " + first_difference(got, want)


# ---------------------------------------------------------------- layouts and shapes
@pytest.mark.parametrize("shape", cases.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_read_volume_after_the_filter_matches_the_reference(vra, ranklib, handles, shape, dtype):
    r = handles[0]
    R = vra.renderer
    vol = cases.random_volume(shape, dtype, 11)
    key = (shape, np.dtype(dtype).name, 11)
    for layout in (R.LAYOUT_LINEAR, R.LAYOUT_BRICKED):
        r.setLayout(layout)
        r.setVolume(vol)
        for op in cases.MORPHOLOGY:
            for radius in cases.MORPHOLOGY_RADII:
                check_voxels(r, ranklib, key, vol, op, radius, f"{shape} {np.dtype(dtype).name} layout {layout}")
                assert r.rankFilter == (op, radius)
        for radius in cases.MEDIAN_RADII:
            check_voxels(r, ranklib, key, vol, MEDIAN, radius, f"{shape} {np.dtype(dtype).name} layout {layout}")
            assert r.rankFilter == (MEDIAN, radius)
    r.setLayout(R.LAYOUT_BRICKED)


@pytest.mark.parametrize("layout", [0, 1], ids=["linear", "bricked"])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_unsigned_extremes_and_the_band_at_the_sign_bit(vra, ranklib, handles, dtype, layout):
    r = handles[0]
    vol = cases.extremes_volume(dtype)
    hi = cases.peak(dtype)
    r.setLayout(layout)
    r.setVolume(vol)
    for op, radius in ((ERODE, (1, 1, 1)), (DILATE, (1, 1, 1)), (ERODE, (0, 2, 0)), (DILATE, (3, 0, 0)), (ERODE, (0, 0, 2)), (OPEN, (1, 2, 1)),
                       (CLOSE, (2, 1, 1)), (MEDIAN, (1, 1, 1)), (MEDIAN, (1, 1, 0)), (MEDIAN, (0, 0, 1))):
        check_voxels(r, ranklib, ("extremes", np.dtype(dtype).name), vol, op, radius, f"layout {layout}")
    r.rankFilterVolume(DILATE, 1)
    got = r.readVolume()
    assert int(got.max()) == hi and int(got[12, 5, 5]) == (hi + 1) // 2          # inside the band: 128 | 32768 beats 127 | 32767
    r.rankFilterVolume(ERODE, 1)
    assert int(r.readVolume()[12, 5, 5]) == (hi + 1) // 2 - 1
    r.setLayout(vra.renderer.LAYOUT_BRICKED)


@pytest.mark.parametrize("n_values", [2, 3])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_median_of_volumes_with_few_distinct_values(vra, ranklib, handles, dtype, n_values):
    r = handles[0]
    shape = (37, 18, 11)
    vol = cases.few_values_volume(shape, dtype, n_values, 40 + n_values)
    assert len(np.unique(vol)) == n_values
    r.setLayout(vra.renderer.LAYOUT_BRICKED)
    r.setVolume(vol)
    for radius in cases.MEDIAN_RADII:
        check_voxels(r, ranklib, ("few", np.dtype(dtype).name, n_values), vol, MEDIAN, radius, f"{n_values} values")


# ---------------------------------------------------------------- the launcher's limits
@pytest.mark.parametrize("name", sorted(cases.LIMIT_CASES))
def test_ring_and_segment_limits_at_the_largest_radius(vra, ranklib, handles, name):
    r = handles[0]
    shape, radius, _ = cases.LIMIT_CASES[name]
    big = shape[0] * shape[1] * shape[2] > 1 << 20
    for dtype in ((np.uint8,) if big else (np.uint8, np.uint16)):
        vol = cases.random_volume(shape, dtype, 50)
        for layout in ((1,) if big else (0, 1)):
            r.setLayout(layout)
            r.setVolume(vol)
            for op in ((ERODE, DILATE) if big else (ERODE, DILATE, OPEN)):
                check_voxels(r, ranklib, (name, np.dtype(dtype).name), vol, op, radius, f"{name} layout {layout}")
    r.setLayout(vra.renderer.LAYOUT_BRICKED)


@pytest.mark.parametrize("name", sorted(cases.TILE_CASES))
def test_tile_seams(vra, ranklib, handles, name):
    r = handles[0]
    shape, radius = cases.TILE_CASES[name]
    ops = (MEDIAN,) if name.startswith("MEDIAN") else (ERODE, DILATE)
    for dtype in (np.uint8, np.uint16):
        vol = cases.random_volume(shape, dtype, 51)
        for layout in (0, 1):
            r.setLayout(layout)
            r.setVolume(vol)
            for op in ops:
                check_voxels(r, ranklib, (name, np.dtype(dtype).name), vol, op, radius, f"{name} layout {layout}")
                if op == MEDIAN:
                    check_voxels(r, ranklib, (name, np.dtype(dtype).name), vol, op, (0, 1, 1), f"{name} layout {layout}")
    r.setLayout(vra.renderer.LAYOUT_BRICKED)


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


# ---------------------------------------------------------------- state
def test_off_restores_the_loaded_volume_and_calls_never_accumulate(vra, oracle, ranklib, handles):
    r = handles[0]
    R = vra.renderer
    dims = (41, 39, 40)
    vol = oracle.gen_noise_ball(dims, 1, 77)
    key = ("ball8", 77)
    r.setLayout(R.LAYOUT_BRICKED)
    r.setVolume(vol)
    r.setWindow(20, 230)
    r.setAlpha(0.3)
    assert r.rankFilter == (R.VR_RANK_OFF, (0, 0, 0))
    before = {}
    for m in MODES:
        set_mode(vra, r, m, dims)
        before[m] = frame(r)
    r.rankFilterVolume(R.VR_RANK_OPEN, (2, 1, 2))
    assert r.rankFilter == (R.VR_RANK_OPEN, (2, 1, 2)) and r.rankFilterMs() > 0.0
    once = r.readVolume()
    assert np.array_equal(once, reference(ranklib, key, vol, OPEN, (2, 1, 2)))
    r.rankFilterVolume(R.VR_RANK_OPEN, (2, 1, 2))                      # the same call twice: the same bytes (an opening of an opening
    assert np.array_equal(r.readVolume(), once)                        # would be the same too, so a different op decides:)
    r.rankFilterVolume(R.VR_RANK_ERODE, 1)
    assert np.array_equal(r.readVolume(), reference(ranklib, key, vol, ERODE, 1))      # ... of the loaded volume, not of the opening
    r.rankFilterVolume(R.VR_RANK_ERODE, 1)
    assert np.array_equal(r.readVolume(), reference(ranklib, key, vol, ERODE, 1))      # an erosion twice would differ
    r.rankFilterVolume(R.VR_RANK_MEDIAN, (1, 1, 0))
    assert np.array_equal(r.readVolume(), reference(ranklib, key, vol, MEDIAN, (1, 1, 0)))
    set_mode(vra, r, "composite", dims)
    assert not np.array_equal(bits(frame(r)[0]), bits(before["composite"][0]))         # the frames do show the filtered volume
    r.rankFilterVolume(R.VR_RANK_OFF, 0)
    assert r.rankFilter == (R.VR_RANK_OFF, (0, 0, 0))
    assert np.array_equal(r.readVolume(), vol)
    for m in MODES:
        set_mode(vra, r, m, dims)
        assert_same_frame(frame(r), before[m], f"{m} after OFF")
    set_mode(vra, r, "composite", dims)
    # OFF with radii, and an op with a box of one voxel, are the identity and read back (OFF, 0, 0, 0)
    r.rankFilterVolume(R.VR_RANK_DILATE, 2)
    r.rankFilterVolume(R.VR_RANK_OFF, (3, 2, 1))
    assert r.rankFilter == (R.VR_RANK_OFF, (0, 0, 0)) and np.array_equal(r.readVolume(), vol)
    r.rankFilterVolume(R.VR_RANK_DILATE, 2)
    r.rankFilterVolume(R.VR_RANK_CLOSE, 0)
    assert r.rankFilter == (R.VR_RANK_OFF, (0, 0, 0)) and np.array_equal(r.readVolume(), vol)


def test_a_refused_call_changes_nothing(vra, oracle, ranklib, handles):
    R = vra.renderer
    fresh = vra.RendererCore(0)
    try:
        fresh.setup((64, 48))
        assert fresh.loadShader("VolumeRenderer.cs")
        with pytest.raises(vra.VRError) as e:
            fresh.rankFilterVolume(R.VR_RANK_ERODE, 1)             # before any volume: what vr_read_volume gives
        assert e.value.code == R.VR_E_INVALID
        assert fresh.rankFilter == (R.VR_RANK_OFF, (0, 0, 0))
    finally:
        fresh.close()
    r = handles[0]
    vol = oracle.gen_noise_ball((24, 20, 22), 1, 5)
    r.setLayout(R.LAYOUT_BRICKED)
    r.setVolume(vol)
    r.setWindow(10, 240)
    r.rankFilterVolume(R.VR_RANK_CLOSE, (1, 2, 0))
    voxels, fr = r.readVolume(), frame(r)
    for op, radius in ((-1, 1), (6, 1), (R.VR_RANK_ERODE, 9), (R.VR_RANK_DILATE, (0, -1, 0)), (R.VR_RANK_OPEN, (0, 0, 9)), (R.VR_RANK_MEDIAN, 2),
                       (R.VR_RANK_MEDIAN, (1, 1, 2)), (R.VR_RANK_OFF, (0, 9, 0))):
        with pytest.raises(vra.VRError) as e:
            r.rankFilterVolume(op, radius)
        assert e.value.code == R.VR_E_INVALID, (op, radius)
        assert r.rankFilter == (R.VR_RANK_CLOSE, (1, 2, 0))
    assert np.array_equal(r.readVolume(), voxels)
    assert_same_frame(frame(r), fr, "after refused calls")
    r.rankFilterVolume(R.VR_RANK_OFF, 0)


def test_a_load_resets_the_state_and_the_kept_volume_is_counted_under_other(vra, oracle, handles):
    r = handles[0]
    R = vra.renderer
    r.setLayout(R.LAYOUT_BRICKED)
    vol = oracle.gen_noise_ball((40, 40, 40), 2, 9)
    r.setVolume(vol)
    v0, c0, o0 = r.residentBytes()
    r.rankFilterVolume(R.VR_RANK_DILATE, (1, 0, 2))
    assert r.residentBytes() == (v0, 0, o0 + v0)                   # the rendered volume; the kept loaded one under `other`; no intermediate left
    r.rankFilterVolume(R.VR_RANK_OPEN, 2)
    assert r.residentBytes() == (v0, 0, o0 + v0)
    r.rankFilterVolume(R.VR_RANK_OFF, 0)
    assert r.residentBytes() == (v0, 0, o0)
    r.rankFilterVolume(R.VR_RANK_MEDIAN, 1)
    r.smoothVolume(sigma_voxels=1.0)
    r.setVolume(vol)
    assert r.rankFilter == (R.VR_RANK_OFF, (0, 0, 0)) and r.smoothing == (0.0, 0.0, 0.0) and r.residentBytes()[2] == o0
    assert np.array_equal(r.readVolume(), vol)
    r.rankFilterVolume(R.VR_RANK_MEDIAN, 1)
    r.generateSynthetic(R.SYNTH_NOISE_BALL, (32, 32, 32), 1, 3)
    assert r.rankFilter == (R.VR_RANK_OFF, (0, 0, 0))
    r.rankFilterVolume(R.VR_RANK_OFF, 0)                           # nothing to drop: a no-op
    assert r.rankFilter == (R.VR_RANK_OFF, (0, 0, 0))


def test_the_labelling_is_dropped_and_the_mesh_is_kept(vra, oracle, handles):
    r = handles[0]
    R = vra.renderer
    vol = oracle.gen_noise_ball((40, 40, 40), 1, 9)
    r.setLayout(R.LAYOUT_BRICKED)
    r.setVolume(vol)
    r.extractIsosurface(100)
    mesh = r.meshInfo()
    assert r.labelComponents(100) > 0
    r.componentsInfo()
    r.rankFilterVolume(R.VR_RANK_MEDIAN, 1)
    assert r.meshInfo() == mesh                                    # a snapshot of the voxels it was extracted from
    with pytest.raises(vra.VRError) as e:
        r.componentsInfo()                                         # a labelling of voxels that are no longer rendered
    assert e.value.code == R.VR_E_INVALID
    assert r.labelComponents(100) > 0                              # of the filtered voxels
    r.rankFilterVolume(R.VR_RANK_OFF, 0)
    with pytest.raises(vra.VRError):
        r.componentsInfo()
    assert r.meshInfo() == mesh
    r.freeComponents()
    r.freeMesh()


def test_set_layout_after_the_filter_relays_both_volumes(vra, ranklib, handles):
    r = handles[0]
    R = vra.renderer
    vol = cases.random_volume((41, 39, 40), np.uint8, 31)
    want = reference(ranklib, ("layout8", 31), vol, CLOSE, (1, 0, 2))
    for first, second in ((R.LAYOUT_BRICKED, R.LAYOUT_LINEAR), (R.LAYOUT_LINEAR, R.LAYOUT_BRICKED)):
        r.setLayout(first)
        r.setVolume(vol)
        r.rankFilterVolume(R.VR_RANK_CLOSE, (1, 0, 2))
        ms = r.rankFilterMs()
        r.setLayout(second)
        assert r.rankFilter == (R.VR_RANK_CLOSE, (1, 0, 2)) and r.rankFilterMs() == ms      # nothing was computed again
        assert np.array_equal(r.readVolume(), want)
        r.rankFilterVolume(R.VR_RANK_OFF, 0)
        assert np.array_equal(r.readVolume(), vol)
    r.setLayout(R.LAYOUT_BRICKED)


# ---------------------------------------------------------------- composition with the Gaussian
def test_composition_with_the_gaussian(vra, ranklib, smoothlib, handles):
    r = handles[0]
    R = vra.renderer
    sig = (1.0, 0.5, 2.0)
    weights = tuple(vra.smooth_weights(s) for s in sig)
    for dtype in (np.uint8, np.uint16):
        vol = cases.random_volume((41, 39, 40), dtype, 61)
        key = ("compose", np.dtype(dtype).name)
        ranked = reference(ranklib, key, vol, MEDIAN, (1, 1, 1))
        both = smooth_ref.smooth(smoothlib, ranked, weights)           # G(R(loaded))
        smoothed = smooth_ref.smooth(smoothlib, vol, weights)
        r.setLayout(R.LAYOUT_BRICKED)
        r.setVolume(vol)
        r.rankFilterVolume(R.VR_RANK_MEDIAN, 1)
        r.smoothVolume(sigma_voxels=sig)
        got = r.readVolume()
        assert np.array_equal(got, both), "rank, then smooth: " + first_difference(got, both)
        assert r.rankFilter == (R.VR_RANK_MEDIAN, (1, 1, 1)) and r.smoothing == sig
        v0 = r.residentBytes()
        # the other order, from the loaded volume again
        r.setVolume(vol)
        r.smoothVolume(sigma_voxels=sig)
        got = r.readVolume()
        assert np.array_equal(got, smoothed), "rank OFF: smoothing alone " + first_difference(got, smoothed)
        r.rankFilterVolume(R.VR_RANK_MEDIAN, 1)
        got = r.readVolume()
        assert np.array_equal(got, both), "smooth, then rank: " + first_difference(got, both)
        assert r.residentBytes() == v0                                 # R's voxels were an intermediate: two volumes stay
        # a different op under the same Gaussian
        r.rankFilterVolume(R.VR_RANK_DILATE, (2, 0, 1))
        want = smooth_ref.smooth(smoothlib, reference(ranklib, key, vol, DILATE, (2, 0, 1)), weights)
        assert np.array_equal(r.readVolume(), want)
        # turning either off leaves the other alone
        r.rankFilterVolume(R.VR_RANK_OFF, 0)
        assert r.smoothing == sig and np.array_equal(r.readVolume(), smoothed)
        r.rankFilterVolume(R.VR_RANK_MEDIAN, 1)
        r.smoothVolume(sigma_voxels=0.0)
        assert r.rankFilter == (R.VR_RANK_MEDIAN, (1, 1, 1)) and r.smoothing == (0.0, 0.0, 0.0)
        assert np.array_equal(r.readVolume(), ranked)
        r.rankFilterVolume(R.VR_RANK_OFF, 0)
        assert np.array_equal(r.readVolume(), vol) and r.residentBytes()[2] < v0[2]


# ---------------------------------------------------------------- derived data
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
    elif case == "trilinear_tf_skip":
        r.setFilter(R.FILTER_TRILINEAR)
        r.setTransferFunction(TF_ISO, TF_RGBA)
        r.setSkipEmpty(True)
    elif case == "mip":
        set_mode(vra, r, "mip", dims)
    elif case == "iso_skip":
        set_mode(vra, r, "iso", dims)
        r.setSkipEmpty(True)
    elif case == "reslice":
        set_mode(vra, r, "reslice", dims)


CASES = ["nearest_pack12", "nearest_tf_skip", "trilinear_tf_skip", "mip", "iso_skip", "reslice"]


@pytest.mark.parametrize("case", CASES)
def test_everything_derived_from_the_voxels_follows_the_filter(vra, ranklib, handles, case):
    """a handle that rendered the loaded volume (so every copy, grid and order of it exists), then filtered it, against a fresh
    handle that was given the CPU-filtered voxels and the same window"""
    r, f = handles
    R = vra.renderer
    dims = (41, 39, 40)
    rng = np.random.default_rng(21)
    # 16-bit data inside a ball, zero outside, with salt (20000) and pepper (0) voxels: the median removes both, so the range
    # shrinks to within 4096 values (the packed copy becomes possible) and the ball's shell and the skip grid's cells move
    zz, yy, xx = np.meshgrid(np.arange(40), np.arange(39), np.arange(41), indexing="ij")
    ball = (xx - 20) ** 2 + (yy - 19) ** 2 + (zz - 20) ** 2 < 15 ** 2
    vol = np.where(ball, rng.integers(1000, 3000, size=ball.shape), 0).astype(np.uint16)
    vol[5::9, 4::9, 3::9] = 20000
    vol[2::9, 6::9, 7::9] = 0
    op, radius = (MEDIAN, (1, 1, 1)) if case != "iso_skip" else (OPEN, (2, 2, 2))
    want = reference(ranklib, ("ball16", 21), vol, op, radius)
    assert int(want.max()) - int(want.min()) <= 4095 < int(vol.max()) - int(vol.min())
    window = (-1000, 3095)                                    # stored 0 .. 4095 under VR_QUIRK_U16_OFFSET
    for r_ in (r, f):
        r_.setLayout(R.LAYOUT_BRICKED)
        configure(vra, r_, case, dims)
    r.setVolume(vol)
    r.setWindow(*window)
    stale = frame(r)
    # (pack12Bytes is the composite and MIP launches' figure: an isosurface or reslice launch leaves the last one standing)
    packs = case not in ("iso_skip", "reslice")
    assert r.pack12Bytes() == 0 or not packs
    r.takeMessage()
    r.rankFilterVolume(op, radius)
    assert r.window == window and r.takeMessage() is None
    f.setVolume(want)
    f.setWindow(*window)
    got, fresh = frame(r), frame(f)
    assert_same_frame(got, fresh, case)
    assert not np.array_equal(bits(got[0]), bits(stale[0]))
    assert r.pack12Bytes() == f.pack12Bytes() or not packs
    if case == "nearest_pack12":
        assert r.pack12Bytes() > 0
    assert r.dataset_range == f.dataset_range
    assert np.array_equal(r.histogram(), f.histogram())
    assert np.array_equal(r.readVolume(), want)
    # the converse: back on the loaded volume nothing built from the filtered one is used again
    r.rankFilterVolume(R.VR_RANK_OFF, 0)
    assert_same_frame(frame(r), stale, f"{case}: the loaded volume after OFF")
    assert r.pack12Bytes() == 0 or not packs
    for r_ in (r, f):
        configure(vra, r_, "nearest_pack12", dims)


def test_the_call_keeps_the_users_state(vra, oracle, handles):
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
    r.rankFilterVolume(R.VR_RANK_DILATE, (1, 2, 0))
    assert r.takeMessage() is None
    assert r.window == (-300, 2500)
    assert np.array_equal(bits(r.getCameraBlock()), bits(cam))
    assert np.array_equal(bits(r.getTransferLut()), bits(lut))
    assert r.shading() == shading and r.dims == dims
    assert not np.array_equal(bits(frame(r)[0]), bits(mip[0]))  # still MIP with TRILINEAR, now of the dilated volume
    r.rankFilterVolume(R.VR_RANK_OFF, 0)
    assert_same_frame(frame(r), mip, "the MIP frame after OFF")
    r.setMIP(False); r.setShading(False); r.setTransferFunction(); r.setFilter(R.FILTER_NEAREST); r.resetCamera()


# ---------------------------------------------------------------- 64-bit offsets
def test_beyond_32_bit_offsets_on_sampled_voxels(vra, ranklib):
    """2048 x 2048 x 1032 u8, bricked: 4.03 GiB of voxels; the storage offset 2^32 is the first voxel of brick layer 256,
    (0, 0, 1024).  ERODE r = 1 (three passes, two buffers beside the loaded volume) and the 3x3x3 MEDIAN on about 2000 voxels
    against the pointwise CPU definition: the first and the last voxel, both sides of the offset, random ones.  Only where four
    volumes fit the free device memory."""
    import torch

    R = vra.renderer
    nx, ny, nz = 2048, 2048, 1032
    free_bytes, _ = torch.cuda.mem_get_info(0)
    if free_bytes < 4 * nx * ny * nz + (2 << 30):
        pytest.skip("four volumes of 4.03 GiB do not fit the free device memory")
    r = vra.RendererCore(0)
    try:
        r.setup((64, 48))
        assert r.loadShader("VolumeRenderer.cs")
        r.setLayout(R.LAYOUT_BRICKED)
        r.generateSynthetic(R.SYNTH_NOISE_BALL, (nx, ny, nz), 1, 0xBEEF)
        vol = r.readVolume()
        rng = np.random.default_rng(32)
        pts = [(0, 0, 0), (nx - 1, ny - 1, nz - 1), (0, 0, 1023), (3, 3, 1023), (nx - 1, ny - 1, 1023), (0, 0, 1024), (1, 0, 1024), (0, 1, 1024),
               (nx - 1, ny - 1, 1024), (0, 0, 1025), (nx - 1, 0, 0), (0, ny - 1, nz - 1)]
        for z in (1021, 1022, 1023, 1024, 1025, 1026, 1031):
            pts += [(int(x), int(y), z) for x, y in rng.integers(0, 2048, size=(80, 2))]
        pts += [(int(x), int(y), int(z)) for x, y, z in zip(rng.integers(0, nx, 1400), rng.integers(0, ny, 1400), rng.integers(0, nz, 1400))]
        ijk = np.asarray(pts, dtype=np.int32)
        for op, name in ((R.VR_RANK_ERODE, "erode"), (R.VR_RANK_MEDIAN, "median")):
            r.rankFilterVolume(op, 1)
            got = r.readVolume()
            want = rank_ref.rank_points(ranklib, vol, op, 1, ijk)
            have = got[ijk[:, 2], ijk[:, 1], ijk[:, 0]]
            del got
            bad = np.flatnonzero(have != want)
            assert bad.size == 0, f"{name}: {bad.size} of {len(pts)} sampled voxels differ, first {tuple(ijk[bad[0]])}: {have[bad[0]]} vs {want[bad[0]]}"
            assert np.any(have != vol[ijk[:, 2], ijk[:, 1], ijk[:, 0]])                  # the samples do see the filter
    finally:
        r.close()
