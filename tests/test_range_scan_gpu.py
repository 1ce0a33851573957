"""The range scan's skipped voxel (linear index 8390640, X) and everything the exact range selects, on the GPU.

stats_kernel pass 0 yields the reference's range (X left out: dataset range, default window, histogram scale) and the exact range
(X included: the 12-bit packed volume copy and its base, the ray stream's 12-bit format and its base, the instances that index
the window table without clamping, the skip-order signature).  tests/range_scan_cases.py has the smallest volumes in which the
two differ -- an extreme value at X -- and cameras zoomed on X; tests/test_range_scan_cpu.py proves from the oracle alone that
every frame rendered here reads X.  Frames are compared bit for bit, and per-pixel sample counts by value, with oracle.render;
the affected pixels of the CPU file are asserted to be among the pixels compared.  Windows are in STORED units (setQuirks(0)).

1  ranges and histogram: three shapes, both layouts, every kind and its twin with the value at index 8390639
2  the packed volume copy: taken when the EXACT span fits, its base the exact minimum
3  the default window straight after a load (it excludes X: that sample must clamp) on every kernel and on replayed frames
4  the ray stream's format and base
5  empty-space skipping with nothing but X above the window's lower end
6  the other ways voxels arrive or change: a RAW file, the synthetic generator, a layout change, smoothing
7  all-zero volumes: a finite histogram
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


C = _load("range_scan_cases", _HERE / "range_scan_cases.py")

GENERIC, FAST, RELAY = "raymarch_generic_kernel", "raymarch_fast_kernel", "raymarch_relay_kernel"
STREAM, STREAM12 = "raymarch_stream_kernel", "raymarch_stream12_kernel"
FASTS = (FAST, RELAY)
TF_KNOTS = ([0, 90, 160, 255], [[0, 0, 0, 0], [0.9, 0.2, 0.1, 0.3], [0.2, 0.8, 0.3, 0.1], [1, 1, 1, 0.9]])   # of test_u16_full_range_gpu.py
FAST_TF_WINDOW_MAX = 28672          # vr_frame.h: the widest window with a transfer-function index table (wider: the generic kernel)
FAST_AXIS_TAB_MAX = 3072            # vr_frame.h: nx + ny + nz up to which the address tables, and with them the packed copy, are used
LINEAR, BRICKED = 0, 1
LAYOUT_IDS = ["linear", "bricked"]

_REFERENCE = {}                     # (shape, kind, at) -> (reference_range, reference_histogram): computed once, shared by the layouts
_WANT = {}                          # oracle frames, computed once and left unchanged
_AFFECTED = {}
_LUT = []


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def reference_of(shape, kind, at=C.SKIPPED_INDEX):
    key = (shape, kind, at)
    if key not in _REFERENCE:
        vol = C.volume_u8(shape) if kind == "u8" else C.volume(shape, kind, at)
        _REFERENCE[key] = (C.reference_range(vol), C.reference_histogram(vol)[0])
    return _REFERENCE[key]


def fresh(vra, size, vol, layout=BRICKED, pack12=1):
    r = vra.RendererCore(0)
    r.setup(size)
    assert r.loadShader("VolumeRenderer.cs")
    r.setQuirks(0)
    r.setPack12(pack12)
    r.setLayout(layout)
    if vol is not None:
        r.setVolume(vol)
    return r


def set_mode(r, mode):
    r.setMIP(mode == "mip")
    if mode == "tf":
        r.setTransferFunction(*TF_KNOTS)
        if not _LUT:
            _LUT.append(r.getTransferLut())
    else:
        r.setTransferFunction()


def aim(r, view, mode="grey", variant=0, skip=False):
    r.setKernelVariant(variant)
    r.setFilter(0)
    set_mode(r, mode)
    r.setSkipEmpty(skip)
    r.setAlpha(view.alpha)
    r.setCameraBlock(C.camera_block(view))


def shoot(r):
    r.render()
    rgba, name = r.readPixels(), r.last_kernel_name
    return rgba, name


def want_frame(oracle, key, vol, view, window, mode):
    """the oracle's frame and per-pixel counts of a case, once; `key` names the volume"""
    k = (key, view.name, window, mode)
    if k not in _WANT:
        if mode == "tf" and not _LUT:
            raise AssertionError("set_mode(r, 'tf') first")
        rgba, _, spp = oracle.render(vol, C.params(oracle, view, window, mode, _LUT[0] if mode == "tf" else None), want_spp=True)
        rgba.setflags(write=False); spp.setflags(write=False)
        _WANT[k] = (rgba, spp)
    return _WANT[k]


def affected(oracle, key, vol, view, window):
    k = (key, view.name, window)
    if k not in _AFFECTED:
        _AFFECTED[k] = C.affected_pixels(oracle, vol, view, window)
    return _AFFECTED[k]


def problems_of(got, want, px, what, spp=None):
    """[] when the frame is the oracle's: the affected pixels lie in the compared frame and agree, and so does everything else"""
    out = []
    rgba, want_rgba = got, want[0]
    if rgba.shape != want_rgba.shape:
        return [f"{what}: shape {rgba.shape} vs {want_rgba.shape}"]
    h, w = rgba.shape[:2]
    if not (len(px) >= 1 and (px[:, 0] < h).all() and (px[:, 1] < w).all() and (px >= 0).all()):
        out.append(f"{what}: the affected pixels {px.tolist()} are not among the {w}x{h} pixels compared")
        return out
    at = (px[:, 0], px[:, 1])
    if not np.array_equal(bits(rgba)[at], bits(want_rgba)[at]):
        out.append(f"{what}: the pixels that read X differ: {rgba[at].tolist()} vs {want_rgba[at].tolist()}")
    bad = bits(rgba) != bits(want_rgba)
    if bad.any():
        first = tuple(int(i) for i in np.argwhere(bad)[0])
        out.append(f"{what}: {int(bad.any(axis=2).sum())} pixels differ, first at {first}: {rgba[first]!r} vs {want_rgba[first]!r}")
    if spp is not None and not np.array_equal(spp, want[1]):
        first = tuple(int(i) for i in np.argwhere(spp != want[1])[0])
        out.append(f"{what}: {int((spp != want[1]).sum())} sample counts differ, first at {first}: {spp[first]} vs {want[1][first]}")
    return out


def expected_kernels(shape, variant, window, mode, skip=False):
    """the kernels a NEAREST frame may report (vr_kernels.hip: launch_raymarch, relay_selected; launch_plan.cpp: fast_path_eligible)"""
    width = window[1] - window[0] + 1
    if variant == 1 or width < 2 or (mode == "tf" and width > FAST_TF_WINDOW_MAX):
        return (GENERIC,)
    if variant in (2, 5):
        return (FAST,)
    table = width <= (FAST_TF_WINDOW_MAX if mode == "tf" else 4096)
    relay = mode == "grey" or (table and sum(C.SHAPES[shape]) <= FAST_AXIS_TAB_MAX)
    if variant == 3:
        return FASTS if skip else ((RELAY,) if relay else (FAST,))
    return FASTS


def finish(problems, frames, at_least):
    assert not problems, f"{len(problems)} problems:\n" + "\n".join(problems[:30])
    assert frames >= at_least, frames


# ---------------------------------------------------------------------------------------------------------------
# 1: ranges and histogram
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [LINEAR, BRICKED], ids=LAYOUT_IDS)
@pytest.mark.parametrize("shape", list(C.SHAPES))
def test_ranges_and_histogram(vra, shape, layout):
    """every kind and its index-8390639 twin: dataset range == default window == the reference's range, which on the shapes with X
    is NOT (vol.min(), vol.max()); the histogram at the reference's scale; the 8-bit twin keeps (0, 255)"""
    cases = [(kind, at) for kind in C.KINDS for at in (C.SKIPPED_INDEX, C.SKIPPED_INDEX - 1)]
    if shape in C.WITH_X:
        cases.append(("u8", C.SKIPPED_INDEX))
    differ = 0
    with fresh(vra, (32, 32), None, layout) as r:
        for kind, at in cases:
            vol = C.volume_u8(shape) if kind == "u8" else C.volume(shape, kind, at)
            want_range, want_hist = reference_of(shape, kind, at)
            r.setVolume(vol)
            what = f"{shape} {kind} value at {at}"
            print(f"{what}: dataset range {r.dataset_range}, window {r.window}, reference {want_range}, exact {C.exact_range(vol)}")
            assert r.dataset_range == r.window == want_range, what
            if kind == "u8":
                assert want_range == (0, 255) and int(vol.max()) == 255
            elif shape in C.WITH_X and at == C.SKIPPED_INDEX:
                assert want_range != C.exact_range(vol), what              # the case exists: the two ranges differ
                differ += 1
            else:
                assert want_range == C.exact_range(vol), what
            got = r.histogram()
            assert got[0] == 0.0 and want_hist[1:].any(), what
            assert np.allclose(got, want_hist, rtol=1e-6, atol=0), (what, np.argwhere(got != want_hist)[:5].ravel(), got[got != want_hist][:5],
                                                                    want_hist[got != want_hist][:5])
    assert differ == (len(C.KINDS) if shape in C.WITH_X else 0)


# ---------------------------------------------------------------------------------------------------------------
# 2: the packed volume copy
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("shape", C.WITH_X)
def test_packed_volume_copy(vra, oracle, shape, kind):
    """bricked, setPack12(1), NEAREST, kernel variants 0, 2, 3, 5, grey composite and MIP, the default and the exact window.  The
    copy exists when the EXACT span fits 12 bits (the reference's span fits for every kind) and the kernel's address tables fit
    (x_plane; on x_last nx + ny + nz > 3072 and no kernel gathers from a copy); it holds voxel - exact minimum"""
    vol = C.volume(shape, kind)
    packs = kind in C.IN_SPAN and sum(C.SHAPES[shape]) <= FAST_AXIS_TAB_MAX
    problems, frames = [], 0
    for view in C.VIEWS_OF[shape]:
        with fresh(vra, view.size, vol) as r:
            for window in (C.default_window(kind), C.exact_window(kind)):
                px = affected(oracle, (shape, kind), vol, view, window)
                r.setWindow(*window)
                for mode in ("grey", "mip"):
                    want = want_frame(oracle, (shape, kind), vol, view, window, mode)
                    for variant in (0, 2, 3, 5):
                        aim(r, view, mode, variant)
                        rgba, name = shoot(r)
                        nbytes = r.pack12Bytes()
                        spp = r.countSamples(per_pixel=True)[1]
                        what = f"{view.name} {kind} window {window} {mode} variant {variant} via {name}, packed copy {nbytes} bytes"
                        problems += problems_of(rgba, want, px, what, spp)
                        if name not in expected_kernels(shape, variant, window, mode):
                            problems.append(f"{what}: unexpected kernel")
                        if (nbytes > 0) != packs:
                            problems.append(f"{what}: a packed copy is {'expected' if packs else 'not allowed'}")
                        frames += 1
    finish(problems, frames, 48)


# ---------------------------------------------------------------------------------------------------------------
# 3: the default window straight after a load
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [LINEAR, BRICKED], ids=LAYOUT_IDS)
@pytest.mark.parametrize("kind", C.IN_SPAN + ("u8",))
@pytest.mark.parametrize("shape", C.WITH_X)
def test_default_window_after_load(vra, oracle, shape, kind, layout):
    """the window is never touched (the 8-bit twin: (0, 200)): every voxel but X lies inside it, so X's sample must clamp -- an
    instance that indexes the window table without clamping is the wrong one.  Variants 0, 1, 2, 3, 5 and a replayed frame;
    grey ramp, transfer function, MIP"""
    vol = C.case_volume(shape, kind)
    window = C.U8_WINDOW if kind == "u8" else reference_of(shape, kind)[0]
    problems, frames = [], 0
    for view in C.VIEWS_OF[shape]:
        with fresh(vra, view.size, vol, layout) as r:
            if kind == "u8":
                r.setWindow(*window)
            assert r.window == window and r.dataset_range == reference_of(shape, kind)[0]
            px = affected(oracle, (shape, kind), vol, view, window)
            for mode in ("grey", "tf", "mip"):
                set_mode(r, mode)
                want = want_frame(oracle, (shape, kind), vol, view, window, mode)
                for variant in (0, 1, 2, 3, 5, "replay"):
                    aim(r, view, mode, 0 if variant == "replay" else variant)
                    r.setRayStream(2 if variant == "replay" else 0)
                    rgba, name = shoot(r)
                    r.setRayStream(0)
                    spp = r.countSamples(per_pixel=True)[1]
                    what = f"{view.name} {kind} {LAYOUT_IDS[layout]} default window {window} {mode} variant {variant} via {name}"
                    problems += problems_of(rgba, want, px, what, spp)
                    allowed = (STREAM, STREAM12) if variant == "replay" else expected_kernels(shape, variant, window, mode)
                    if name not in allowed:
                        problems.append(f"{what}: unexpected kernel")
                    frames += 1
            assert r.window == window
    finish(problems, frames, 54)


# ---------------------------------------------------------------------------------------------------------------
# 4: the ray stream
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [LINEAR, BRICKED], ids=LAYOUT_IDS)
@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("shape", C.WITH_X)
def test_ray_stream_format_and_base(vra, oracle, shape, kind, layout):
    """setRayStream(2) with setRayStreamPack(2 | 0) x setRayStreamTable(0 | 2): an exact span within 12 bits replays from the
    packed kernel (base: the exact minimum), anything wider from the 16-bit one; every replayed frame is the oracle's and the
    gather kernels'"""
    vol = C.volume(shape, kind)
    problems, frames = [], 0
    for view in C.VIEWS_OF[shape]:
        with fresh(vra, view.size, vol, layout) as r:
            for window in (C.default_window(kind), C.exact_window(kind)):
                px = affected(oracle, (shape, kind), vol, view, window)
                r.setWindow(*window)
                for mode in ("grey", "mip", "tf"):
                    if mode == "tf" and window[1] - window[0] + 1 > FAST_TF_WINDOW_MAX:
                        continue                                         # (the generic kernel's frame: nothing to replay)
                    aim(r, view, mode)
                    want = want_frame(oracle, (shape, kind), vol, view, window, mode)
                    r.setRayStream(0)
                    gather, gname = shoot(r)
                    if gname not in FASTS:
                        problems.append(f"{view.name} {kind} window {window} {mode}: gather frame via {gname}")
                    for pack in (2, 0):
                        for table in (0, 2):
                            r.setRayStreamPack(pack)
                            r.setRayStreamTable(table)
                            r.setRayStream(2)
                            rgba, name = shoot(r)
                            r.setRayStream(0)
                            what = f"{view.name} {kind} {LAYOUT_IDS[layout]} window {window} {mode} pack {pack} table {table} via {name}"
                            problems += problems_of(rgba, want, px, what)
                            if not np.array_equal(bits(rgba), bits(gather)):
                                problems.append(f"{what}: not the gather kernels' frame")
                            if name != (STREAM12 if pack == 2 and kind in C.IN_SPAN else STREAM):
                                problems.append(f"{what}: the wrong stream format")
                            frames += 1
    finish(problems, frames, 3 * 2 * 2 * 4)


# ---------------------------------------------------------------------------------------------------------------
# 5: skipping
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [LINEAR, BRICKED], ids=LAYOUT_IDS)
@pytest.mark.parametrize("shape", C.WITH_X)
def test_skipping_keeps_the_cell_of_x(vra, oracle, shape, layout):
    """high_out under a window whose lower end lies above the whole background and at or below X: every cell but X's
    neighbourhood classifies to nothing (x_plane: X's cell is in the partial last layer of cells), and the pixels that read X
    are the only lit ones"""
    kind = "high_out"
    vol = C.volume(shape, kind)
    window = C.skip_window(kind)
    problems, frames = [], 0
    for view in C.VIEWS_OF[shape]:
        with fresh(vra, view.size, vol, layout) as r:
            px = affected(oracle, (shape, kind), vol, view, window)
            r.setWindow(*window)
            for mode in ("grey", "mip", "tf"):
                set_mode(r, mode)
                want = want_frame(oracle, (shape, kind), vol, view, window, mode)
                for variant in (0, 1, 2, 3, 5):
                    aim(r, view, mode, variant, skip=True)
                    rgba, name = shoot(r)
                    spp = r.countSamples(per_pixel=True)[1]
                    what = f"{view.name} {LAYOUT_IDS[layout]} window {window} {mode} variant {variant} skipping via {name}"
                    problems += problems_of(rgba, want, px, what, spp)
                    if name not in expected_kernels(shape, variant, window, mode, skip=True):
                        problems.append(f"{what}: unexpected kernel")
                    if mode != "tf" and not (rgba[px[:, 0], px[:, 1], 3] > 0).all():
                        problems.append(f"{what}: a pixel that reads X is empty")
                    if mode != "tf" and int((rgba[..., 3] > 0).sum()) != len(px):
                        problems.append(f"{what}: {int((rgba[..., 3] > 0).sum())} lit pixels, {len(px)} read X")
                    frames += 1
    finish(problems, frames, 45)


# ---------------------------------------------------------------------------------------------------------------
# 6: the other ways voxels arrive or change (x_plane)
# ---------------------------------------------------------------------------------------------------------------
def check_state(r, oracle, key, vol, kind_window, packs, what, layout=BRICKED):
    """ranges, then one fast-kernel frame per view position of the handle's size: the packing decision and the oracle's frame"""
    view = C.VIEWS_OF["x_plane"][0]
    assert r.dataset_range == C.reference_range(vol), (what, r.dataset_range)
    r.setWindow(*kind_window)
    aim(r, view, "grey", 2)
    rgba, name = shoot(r)
    spp = r.countSamples(per_pixel=True)[1]
    assert name == FAST, (what, name)
    assert (r.pack12Bytes() > 0) == (packs and layout == BRICKED), (what, r.pack12Bytes())
    px = affected(oracle, key, vol, view, kind_window)
    problems = problems_of(rgba, want_frame(oracle, key, vol, view, kind_window, "grey"), px, what, spp)
    assert not problems, problems


@pytest.mark.parametrize("kind", ["high_in_span", "high_out"])
def test_raw_file_with_sidecar(vra, oracle, tmp_path, kind):
    shape = "x_plane"
    vol = C.volume(shape, kind)
    raw = tmp_path / "scan.raw"
    vol.tofile(raw)
    nx, ny, nz = C.SHAPES[shape]
    (tmp_path / "scan.raw.inf").write_text(f"#dimensions\n{nx} {ny} {nz}\n\n#voxel-spacing\n1 1 1\n")
    with fresh(vra, C.VIEWS_OF[shape][0].size, None) as r:
        r.readVolumeData(raw, 2)
        assert r.dims[0] == (nx, ny, nz)
        assert r.dataset_range == r.window == reference_of(shape, kind)[0] != C.exact_range(vol)
        assert np.allclose(r.histogram(), reference_of(shape, kind)[1], rtol=1e-6, atol=0)
        check_state(r, oracle, (shape, kind), vol, C.default_window(kind), kind in C.IN_SPAN, f"RAW file {kind}")


@pytest.mark.parametrize("layout", [LINEAR, BRICKED], ids=LAYOUT_IDS)
def test_synthetic_noise_ball(vra, layout):
    """generateSynthetic writes the voxels on the device: the ranges against the reference's scan of the read-back voxels"""
    with fresh(vra, (32, 32), None, layout) as r:
        r.generateSynthetic(1, C.SHAPES["x_plane"], 2, 20261021)
        vol = r.readVolume()
        assert vol.shape == C.SHAPES["x_plane"][::-1] and vol.dtype == np.uint16
        assert r.dataset_range == r.window == C.reference_range(vol)
        assert np.allclose(r.histogram(), C.reference_histogram(vol)[0], rtol=1e-6, atol=0)


@pytest.mark.parametrize("kind", ["low_in_span", "high_out"])
def test_layout_change_keeps_ranges_and_decisions(vra, oracle, kind):
    shape = "x_plane"
    vol = C.volume(shape, kind)
    with fresh(vra, C.VIEWS_OF[shape][0].size, vol, BRICKED) as r:
        for step, layout in enumerate((BRICKED, LINEAR, BRICKED, LINEAR, BRICKED)):
            r.setLayout(layout)
            assert r.dataset_range == reference_of(shape, kind)[0]
            if step == 0:
                assert r.window == r.dataset_range
            for window in (C.default_window(kind), C.exact_window(kind)):
                check_state(r, oracle, (shape, kind), vol, window, kind in C.IN_SPAN, f"{kind} step {step} layout {layout} window {window}", layout)
            assert np.allclose(r.histogram(), reference_of(shape, kind)[1], rtol=1e-6, atol=0)


@pytest.mark.parametrize("layout", [LINEAR, BRICKED], ids=LAYOUT_IDS)
def test_smoothing_a_peak_at_x(vra, oracle, layout):
    """a flat background of 1000 with 21000 at X: the loaded exact span (20000) forbids packing; smoothVolume(1, 1, 1) leaves a
    peak at X that is the unique maximum, within 12 bits of the floor, and again invisible to the reference's scan"""
    shape = "x_plane"
    vol = C.flat_with_peak(shape, 1000, 21000)
    user = (900, 1500)
    i, j, k = C.x_of(shape)
    with fresh(vra, C.VIEWS_OF[shape][0].size, vol, layout) as r:
        assert r.dataset_range == r.window == (1000, 1000)
        check_state(r, oracle, "peak", vol, user, False, "loaded", layout)
        r.smoothVolume((1.0, 1.0, 1.0))
        smooth = r.readVolume()
        peak = int(smooth[k, j, i])
        assert peak == int(smooth.max()) and np.count_nonzero(smooth == peak) == 1          # the unique maximum sits at X
        assert 0 < peak - int(smooth.min()) <= 4095
        print(f"smoothed: peak {peak}, reference range {C.reference_range(smooth)}, exact {C.exact_range(smooth)}")
        assert C.reference_range(smooth) != C.exact_range(smooth)
        assert r.window == user                                                              # the window stays the user's
        check_state(r, oracle, "smoothed", smooth, user, True, "smoothed", layout)            # (it sets the same window again)
        assert r.dataset_range == C.reference_range(smooth)
        r.smoothVolume((0.0, 0.0, 0.0))
        assert np.array_equal(r.readVolume(), vol)
        assert r.dataset_range == (1000, 1000) and r.window == user
        check_state(r, oracle, "peak", vol, user, False, "restored", layout)


# ---------------------------------------------------------------------------------------------------------------
# 7: all-zero volumes
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [LINEAR, BRICKED], ids=LAYOUT_IDS)
@pytest.mark.parametrize("x_value", [0, 300], ids=["all_zero", "zero_but_x"])
def test_zero_volume_has_a_finite_histogram(vra, oracle, x_value, layout):
    """The reference's scale is 0 here and its own arithmetic undefined (std::round of NaN or infinity stored to uint16_t, then
    0 / 0).  Decided: the dataset range is (0, 0), the histogram is all 0.0, and a frame at the default window renders (the
    degenerate window's frame of zeros, as the oracle defines it).
    Before the guard in RendererCore::computeHistogram: bins 1 .. 255 were NaN (0 * 100 / 0)."""
    shape = "x_plane"
    vol = C.zeros_but_x(shape, x_value)
    view = C.VIEWS_OF[shape][0]
    with fresh(vra, view.size, vol, layout) as r:
        assert r.dataset_range == r.window == (0, 0) == C.reference_range(vol)
        got = r.histogram()
        print(f"histogram of a zero volume (X = {x_value}): finite {bool(np.isfinite(got).all())}, non-zero bins {int(np.count_nonzero(got))}")
        assert np.isfinite(got).all() and not got.any(), got[:8]
        for variant in (0, 1):
            aim(r, view, "grey", variant)
            rgba, name = shoot(r)
            spp = r.countSamples(per_pixel=True)[1]
            want, _, want_spp = oracle.render(vol, C.params(oracle, view, (0, 0)), want_spp=True)
            assert np.array_equal(bits(rgba), bits(want)) and np.array_equal(spp, want_spp), (variant, name)
            assert not rgba.any()


def test_zero_u8_volume_has_a_finite_histogram(vra):
    """8 bits: the normaliser starts at -1 and the largest count raises it to 0 -- the same 0 / 0 (the reference keeps -1 and
    stores -0.0).  A small volume: no voxel at X is needed"""
    with fresh(vra, (32, 32), np.zeros((5, 7, 9), dtype=np.uint8)) as r:
        assert r.dataset_range == r.window == (0, 255)
        got = r.histogram()
        assert np.isfinite(got).all() and not got.any(), got[:8]
