"""16-bit volumes over the whole value range on every kernel.

The rest of the suite draws its u16 voxels from [0, 4096); here every volume has voxels above 4095 (tests/u16_volumes.py: `scaled`
= 16 x a 12-bit field, `white` = uniform in [0, 65536) with a 0 and a 65535, `shifted` = a 12-bit field + 12345 or 61440).  Two
independent handles on the truth: the CPU definitions bit for bit (oracle.render, tests/iso_ref, tests/reslice_ref,
tests/shade_ref), and two exact invariances that tie a full-range frame to a 12-bit one -- 16 * V under the window 16 * [lo, hi]
is V under [lo, hi] (both filters), V + B under [lo, hi] + B is V under [lo, hi] (NEAREST; a reslice mean over more than one
sample excluded) -- see tests/test_u16_full_range_cpu.py, which shows that the CPU definitions satisfy both.

Windows and iso values are in STORED units; handles run with setQuirks(0) unless a case says that it converts through the +1000
of VR_QUIRK_U16_OFFSET.  Every comparison is on RGBA bits and per-pixel counts (and depth / value bits where the mode has them).
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
u16 = _load("u16_volumes", _HERE / "u16_volumes.py")

GENERIC, FAST, RELAY, TRI, TSLAB = ("raymarch_generic_kernel", "raymarch_fast_kernel", "raymarch_relay_kernel", "raymarch_tri_kernel",
                                    "raymarch_tslab_kernel")
ISO, RESLICE, SHADE = "raymarch_iso_kernel", "reslice_kernel", "raymarch_shade_kernel"
FASTS = (FAST, RELAY)
TF_KNOTS = ([0, 90, 160, 255], [[0, 0, 0, 0], [0.9, 0.2, 0.1, 0.3], [0.2, 0.8, 0.3, 0.1], [1, 1, 1, 0.9]])
TF_ISO = [0, 60, 140, 255]
TF_RGBA = [[0.2, 0.9, 0.1, 0.0], [0.9, 0.3, 0.2, 0.4], [1.0, 0.8, 0.6, 0.8], [0.5, 0.5, 1.0, 1.0]]
COEFS = [(0.15, 0.65, 0.2, 16), (1.0, 0.0, 0.0, 16), (0.3, 1.7, 0.6, 1), (0.0, 0.9, 0.35, 128), (0.05, 0.4, 0.9, 2)]     # of test_shading_gpu.py
MODES = {"composite": dict(), "mip": dict(mip=1), "tf": dict(tf=1), "mip_tf": dict(mip=1, tf=1), "accum": dict(accum=1)}
VIEWS = ("front", "top", "bottom")
ALPHAS = (0.02, 0.3, 1.0)
FAST_TF_WINDOW_MAX = 28672           # vr_frame.h: the widest window the transfer-function index-byte table is built for

FRAMES = {}                          # test name -> full-range frames compared (printed when the module is done)


def teardown_module(module):
    print(f"\nfull-range frames compared: {sum(FRAMES.values())} {FRAMES}")


@pytest.fixture(scope="session")
def isolib(tmp_path_factory):
    return iso_ref.build(tmp_path_factory.mktemp("iso_ref_u16_gpu"))


@pytest.fixture(scope="session")
def rslib(tmp_path_factory):
    return reslice_ref.build(tmp_path_factory.mktemp("reslice_ref_u16_gpu"))


@pytest.fixture(scope="session")
def shadelib(tmp_path_factory):
    return shade_ref.build(tmp_path_factory.mktemp("shade_ref_u16_gpu"))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def differ(got, want):
    """'' when the tuples agree (float32 arrays by bits, integer arrays by value), else what differs"""
    out = []
    for k, (g, w) in enumerate(zip(got, want)):
        bad = (bits(g) != bits(w)) if g.dtype == np.float32 else (g != w)
        if bad.any():
            at = tuple(int(i) for i in np.argwhere(bad)[0])
            out.append(f"array {k}: {int(bad.sum())} entries differ, first at {at}: {g[at]} vs {w[at]}")
    return "; ".join(out)


def orbit_cam(oracle, zenith=0.0, azimuth=0.0, zoom_in=0):
    c = oracle.Camera()
    for _ in range(zoom_in):
        c.orient(1.0, 0.0, 0.0)
    if zenith or azimuth:
        c.orient(0.0, zenith, azimuth)
    return c.block()


def cameras(oracle):
    """three outside the box, one inside it, one whose rays are parallel to an axis"""
    out = [("orbit_a", orbit_cam(oracle, 0.42, 0.54)), ("orbit_b", orbit_cam(oracle, -0.9, 1.86)), ("orbit_neg", orbit_cam(oracle, 0.0, -0.3))]
    b = oracle.default_camera_block().copy()
    b[12:15] = b[16:19] = (0.1, 0.05, 0.3)
    out.append(("inside", b))
    b = oracle.default_camera_block().copy()
    b[12:15] = b[16:19] = (0.17, 0.0, 3.0)
    out.append(("axis", b))
    return out


class Scene:
    """one handle, one resident volume; frame() sets every switch of the composite modes, want() is the oracle's frame of it"""

    def __init__(self, vra, oracle, vol, size, spacing=(1.0, 1.0, 1.0), layout=1, pack=1, quirks=0):
        self.vra, self.oracle, self.vol, self.size, self.spacing, self.quirks = vra, oracle, vol, size, spacing, quirks
        self.r = r = vra.RendererCore(0)
        r.setup(size)
        assert r.loadShader("VolumeRenderer.cs")
        r.setQuirks(quirks)
        r.setPack12(pack)
        r.setLayout(layout)
        r.setVolume(vol, spacing)
        self.lut = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.r.close()

    def frame(self, win, alpha, cam, variant=0, filt=0, mip=0, tf=0, accum=0, skip=0, view="front"):
        r = self.r
        r.setKernelVariant(variant)
        r.setFilter(filt)
        r.setMIP(bool(mip))
        r.setTransferFunction(*TF_KNOTS) if tf else r.setTransferFunction()
        if tf and self.lut is None:
            self.lut = r.getTransferLut()
        r.setAccum(accum)
        r.setSkipEmpty(bool(skip))
        r.setInitialCameraRotation(view == "top", view == "bottom")
        r.setWindow(*win)
        r.setAlpha(alpha)
        r.setCameraBlock(cam)
        r.render()
        rgba = r.readPixels()
        name = r.last_kernel_name
        _, spp = r.countSamples(per_pixel=True)
        return (rgba, spp), name

    def want(self, win, alpha, cam, variant=0, filt=0, mip=0, tf=0, accum=0, skip=0, view="front"):
        off = 1000 if self.quirks & self.vra.renderer.QUIRK_U16_OFFSET else 0
        p = self.oracle.OracleParams(self.size[0], self.size[1], cam=cam, alpha_scale=alpha, voxel_size=self.spacing, min_val=win[0] + off,
                                     max_val=win[1] + off, is_mip=int(mip), view_top=int(view == "top"), view_bottom=int(view == "bottom"),
                                     filter=filt, accum=accum, tf_rgba=self.lut if tf else None)
        rgba, _, spp = self.oracle.render(self.vol, p, want_spp=True)
        return rgba, spp


def allowed_kernels(variant, filt, layout, win, mip=0, tf=0, accum=0, skip=0, view="front", **_):
    """the kernels a frame may report: one name wherever the variant forces a family and the configuration is one of its own"""
    width = win[1] - win[0] + 1
    table = 2 <= width <= (FAST_TF_WINDOW_MAX if tf else 4096)          # the window has a classification table in LDS
    if variant == 1 or accum or win[1] <= win[0]:
        return (GENERIC,)
    if filt == 0:
        if tf and width > FAST_TF_WINDOW_MAX:
            return (GENERIC,)                       # no table for the window: the transfer function is classified line by line
        # the relay kernel has the grey composite of the default view in every shape and the other modes and views with a table;
        # a launch that skips through an active grid stays with the fast kernel (vr_kernels.hip: relay_selected)
        relay = (RELAY, FAST) if skip else ((RELAY,) if table or not (mip or tf or view != "front") else (FAST,))
        return {0: FASTS, 2: (FAST,), 3: relay, 5: (FAST,)}[variant]
    if layout == 0:
        return (GENERIC,) if tf else (TRI, GENERIC)  # the staged kernel and the apron copy belong to the bricked layout
    if variant == 0:
        return (TSLAB, GENERIC) if tf else (TSLAB, TRI)   # the staged kernel where the view suits it
    if variant == 2:
        return (GENERIC,) if tf else (TRI,)
    return (TSLAB,)


def variants_of(filt):
    return (0, 1, 2, 3, 5) if filt == 0 else (0, 1, 2, 6, 7, 8, 9, 10, 11)


# ---------------------------------------------------------------------------------------------------------------
# items 1 and 3: every composite kernel family on full-range data, against the oracle and against the 12-bit twin
# ---------------------------------------------------------------------------------------------------------------
TWIN_WINDOWS = [(64, 4095), (1500, 3900), (0, 4095), (2500, 3900)]          # x 16: 64 512, 38 416, 65 536 and 22 416 values wide
WHITE_WINDOWS = [(0, 65535), (20000, 60000), (30000, 34095), (9000, 35000)]


@pytest.mark.parametrize("variant", [0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11],
                         ids=["auto", "generic", "plain", "relay", "pipelined", "staged", "unstaged", "half", "halftall", "three", "small"])
def test_composite_kernel_families(vra, oracle, variant):
    """per layout: a `scaled` volume (with its 12-bit twin on a second handle, packed), a `white` and a `shifted` one; every mode,
    the three views, skipping on and off, three opacities, cameras outside / inside / axis-parallel"""
    cams = cameras(oracle)
    problems, seen, lit, n = [], set(), 0, 0
    for layout in (0, 1):
        dims, size = ((45, 38, 41), (96, 80)) if layout == 0 else ((37, 50, 23), (75, 53))
        spacings = ((1.0, 1.0, 1.0), (1.0, 0.7, 1.9)) if layout == 0 else ((1.0, 1.1, 0.9), (1.0, 1.0, 1.0))
        sc = u16.make(oracle, ("scaled_ball", "scaled_smooth")[layout], dims, 100 + variant)
        wh = u16.make(oracle, "white", dims, 200 + variant)
        sh = u16.make(oracle, f"shifted{u16.SHIFTS[layout]}", dims, 300 + variant)
        with Scene(vra, oracle, sc.vol, size, spacings[0], layout) as s_full, Scene(vra, oracle, sc.twin, size, spacings[0], layout) as s_twin, \
                Scene(vra, oracle, wh.vol, size, spacings[1], layout) as s_white, Scene(vra, oracle, sh.vol, size, spacings[0], layout) as s_shift, \
                Scene(vra, oracle, sh.twin, size, spacings[0], layout) as s_shift_twin:
            k = 0
            for filt in (0, 1):
                if variant not in variants_of(filt):
                    continue
                for mode, mkw in MODES.items():
                    for c in range(3):
                        name, cam = (cams[k % 3], cams[3], cams[4])[c]
                        kw = dict(alpha=ALPHAS[(k + c) % 3], cam=cam, variant=variant, filt=filt, skip=(k // 2 + c) % 2, view=VIEWS[(k + c + layout) % 3], **mkw)
                        lo, hi = TWIN_WINDOWS[(k + c) % 4]
                        what = f"variant {variant} layout {layout} filter {filt} {mode} camera {name} skip {kw['skip']} view {kw['view']} alpha {kw['alpha']}"
                        # 16 * V: against the oracle, and against V itself (unpacked with float classification or the large table vs packed with the LDS table)
                        win = u16.twin_window(sc, lo, hi)
                        full, kname = s_full.frame(win, **kw)
                        seen.add(kname)
                        lit += int((full[0][..., 3] > 0).sum())
                        d = differ(full, s_full.want(win, **kw))
                        if d:
                            problems.append(f"{what} scaled window {win} via {kname} vs oracle: {d}")
                        if kname not in allowed_kernels(layout=layout, win=win, **kw):
                            problems.append(f"{what} scaled window {win}: ran {kname}")
                        if s_full.r.pack12Bytes() != 0:
                            problems.append(f"{what}: a packed copy of a volume spanning {int(sc.vol.max()) - int(sc.vol.min())} values")
                        twin, tname = s_twin.frame((lo, hi), **kw)
                        d = differ(full, twin)
                        if d:
                            problems.append(f"{what} scaled window {win} via {kname} vs the 12-bit twin via {tname}: {d}")
                        if (s_twin.r.pack12Bytes() > 0) != (layout == 1 and tname in FASTS):
                            problems.append(f"{what}: twin via {tname}, packed copy of {s_twin.r.pack12Bytes()} bytes")
                        # white
                        win = WHITE_WINDOWS[(k + c) % 4]
                        white, kname = s_white.frame(win, **kw)
                        seen.add(kname)
                        lit += int((white[0][..., 3] > 0).sum())
                        d = differ(white, s_white.want(win, **kw))
                        if d:
                            problems.append(f"{what} white window {win} via {kname} vs oracle: {d}")
                        if kname not in allowed_kernels(layout=layout, win=win, **kw):
                            problems.append(f"{what} white window {win}: ran {kname}")
                        if s_white.r.pack12Bytes() != 0:
                            problems.append(f"{what}: a packed copy of a white volume")
                        n += 2
                        # V + B (NEAREST): against the oracle and against V
                        if filt == 0:
                            win = u16.twin_window(sh, lo, hi)
                            shifted, kname = s_shift.frame(win, **kw)
                            seen.add(kname)
                            d = differ(shifted, s_shift.want(win, **kw))
                            if d:
                                problems.append(f"{what} {sh.kind} window {win} via {kname} vs oracle: {d}")
                            d = differ(shifted, s_shift_twin.frame((lo, hi), **kw)[0])
                            if d:
                                problems.append(f"{what} {sh.kind} window {win} via {kname} vs the 12-bit twin: {d}")
                            if (s_shift.r.pack12Bytes() > 0) != (layout == 1 and kname in FASTS):
                                problems.append(f"{what}: {sh.kind} via {kname}, packed copy of {s_shift.r.pack12Bytes()} bytes")
                            n += 1
                        k += 1
    FRAMES[f"families[{variant}]"] = n
    assert not problems, f"{len(problems)} problems:\n" + "\n".join(problems[:40])
    assert lit > 1000, lit
    forced = {1: {GENERIC}, 2: {FAST, TRI, GENERIC}, 3: {RELAY, FAST, GENERIC}, 5: {FAST, GENERIC}}.get(variant)
    if forced:
        assert seen == forced, seen
    elif variant >= 6:
        assert TSLAB in seen and seen <= {TSLAB, TRI, GENERIC}, seen
    else:
        assert seen & set(FASTS) and seen & {TSLAB, TRI}, seen


# ---------------------------------------------------------------------------------------------------------------
# item 2: window and table boundaries
# ---------------------------------------------------------------------------------------------------------------
WINDOWS = [
    ("ramp_4096", (30000, 34095), 0, 0),          # the last window with the (c, a) table
    ("ramp_4097", (30000, 34096), 0, 0),          # the first without it
    ("tf_28672", (20000, 48671), 1, 0),           # FAST_TF_WINDOW_MAX: the last window with the index-byte table
    ("tf_28673", (20000, 48672), 1, 0),
    ("top_4096", (61440, 65535), 0, 0),
    ("top_4096_tf", (61440, 65535), 1, 0),
    ("whole", (0, 65535), 0, 0),
    ("whole_tf", (0, 65535), 1, 0),
    ("top_2", (65534, 65535), 0, 0),
    ("top_2_tf", (65534, 65535), 1, 0),
    ("degenerate", (65535, 65535), 0, 0),
    ("quirk_whole", (0, 65535), 0, 1),            # uploaded as [1000, 66535]: the maximum lies above any voxel
    ("quirk_whole_tf", (0, 65535), 1, 1),
]


@pytest.mark.parametrize("name,win,tf,quirk", WINDOWS, ids=[w[0] for w in WINDOWS])
def test_window_and_table_boundaries(vra, oracle, name, win, tf, quirk):
    R = vra.renderer
    dims, size = (45, 38, 41), (96, 80)
    cams = cameras(oracle)
    problems, lit, n = [], 0, 0
    for kind, seed in (("scaled_ball", 7), ("white", 8)):
        v = u16.make(oracle, kind, dims, seed)
        with Scene(vra, oracle, v.vol, size, quirks=R.QUIRK_U16_OFFSET if quirk else 0) as s:
            up = (win[0] + 1000, win[1] + 1000) if quirk else win
            for variant, filt in ((2, 0), (3, 0), (6, 1)):
                for skip in (0, 1):
                    kw = dict(alpha=0.3, cam=cams[(variant + skip) % 3][1], variant=variant, filt=filt, tf=tf, skip=skip)
                    got, kname = s.frame(win, **kw)
                    what = f"{name} {kind} variant {variant} filter {filt} skip {skip} via {kname}"
                    d = differ(got, s.want(win, **kw))
                    if d:
                        problems.append(f"{what} vs oracle: {d}")
                    if kname not in allowed_kernels(layout=1, win=up, **kw):
                        problems.append(f"{what}: unexpected kernel")
                    if s.r.pack12Bytes() != 0:
                        problems.append(f"{what}: packed copy")
                    if name == "degenerate" and got[0].any():
                        problems.append(f"{what}: max == min must give a frame of zeros")
                    lit += int((got[0][..., 3] > 0).sum())
                    n += 1
    FRAMES[f"windows[{name}]"] = n
    assert not problems, f"{len(problems)} problems:\n" + "\n".join(problems[:40])
    if name not in ("top_2", "top_2_tf", "degenerate"):
        assert lit > 280, lit              # twelve frames, each of which the oracle lights at 280 pixels or more


# ---------------------------------------------------------------------------------------------------------------
# item 4: isosurface
# ---------------------------------------------------------------------------------------------------------------
def hip_iso(r):
    r.render()
    return r.readPixels(), r.readDepth(), r.countSamples(per_pixel=True)[1]


def test_isosurface_matrix(vra, oracle, isolib):
    rng = np.random.default_rng(20261101)
    poses = [dict(), dict(zenith=0.5, azimuth=0.8), dict(zenith=-0.7, azimuth=2.2), dict(zoom_in=3), dict(zoom_in=2, zenith=0.3, azimuth=-0.4),
             dict(zenith=1.2, azimuth=0.1)]
    kinds = ("scaled_ball", "white", "scaled_smooth", "white", "scaled_rand", "scaled_ball")
    problems, hits, misses, n = [], 0, 0, 0
    r, t = vra.RendererCore(0), vra.RendererCore(0)          # t: the 12-bit twin's handle
    try:
        for case in range(63):
            dims = tuple(int(v) for v in rng.integers(9, 48, size=3))
            if case % 5 == 0:
                dims = (dims[0] | 1, dims[1], dims[2])
            spacing = (1.0, 1.0, 1.0) if rng.integers(3) == 0 else tuple(float(v) for v in rng.uniform(0.5, 2.0, size=3).round(2))
            w, h = int(rng.integers(17, 70)), int(rng.integers(17, 70))
            v = u16.make(oracle, kinds[case % len(kinds)], dims, int(rng.integers(1 << 31)))
            vmin, vmax = int(v.vol.min()), int(v.vol.max())
            stored = [vmin - 1, vmin, (vmin + vmax) // 2 // v.scale * v.scale, vmax, vmax + 1, 65535, 65536][case % 7]
            quirk = case % 2 == 1                                   # odd cases convert: the iso value and the window go in as stored - 1000
            off = 1000 if quirk else 0
            view = VIEWS[int(rng.integers(3))]
            filt, layout, accum = (int(x) for x in rng.integers(2, size=3))
            use_tf = rng.integers(2) == 1
            lo, hi = int(rng.integers(0, 1300)) * 16, int(rng.integers(2000, 4096)) * 16
            cam = orbit_cam(oracle, **poses[int(rng.integers(len(poses)))])
            frames = {}
            for skip in (False, True):
                for handle, vol, scale in ((r, v.vol, 1), (t, v.twin, v.scale)):
                    if vol is None or (handle is t and skip):
                        continue
                    handle.setup((w, h))
                    assert handle.loadShader("VolumeRenderer.cs")
                    handle.setQuirks(vra.renderer.QUIRK_U16_OFFSET if quirk else 0)
                    handle.setLayout(layout)
                    handle.setVolume(vol, spacing)
                    handle.setInitialCameraRotation(view == "top", view == "bottom")
                    handle.setCameraBlock(cam)
                    handle.setFilter(filt)
                    handle.setAccum(accum)
                    handle.setWindow(lo // scale - off, hi // scale - off)
                    handle.setSkipEmpty(skip)
                    handle.setTransferFunction(TF_ISO, TF_RGBA) if use_tf else handle.setTransferFunction()
                    # (scaled: stored is a multiple of 16 or one of the edge values; the twin's iso is the exact quotient when there is one)
                    handle.setIsosurface(True, stored // scale - off)
                    frames[(handle is t, skip)] = hip_iso(handle)
                    assert handle.last_kernel_name == ISO
            what = (f"case {case}: {v.kind} {dims} {spacing} {w}x{h} stored iso {stored} in [{vmin}, {vmax}] {view} filt {filt} layout {layout} accum {accum} "
                    f"tf {use_tf} quirk {quirk}")
            p = oracle.OracleParams(w, h, cam=cam, voxel_size=spacing, min_val=lo, max_val=hi, view_top=int(view == "top"),
                                    view_bottom=int(view == "bottom"), filter=filt, accum=accum, tf_rgba=r.getTransferLut() if use_tf else None)
            want = iso_ref.render(isolib, v.vol, p, stored - off, u16_offset=quirk)
            for skip in (False, True):
                d = differ(frames[(False, skip)], want)
                if d:
                    problems.append(f"{what} skip {skip} vs reference: {d}")
            if v.twin is not None and stored % v.scale == 0:
                d = differ(frames[(False, False)], frames[(True, False)])
                if d:
                    problems.append(f"{what} vs the 12-bit twin at iso {stored // v.scale}: {d}")
            hit = np.isfinite(frames[(False, True)][1])
            hits += int(hit.any())
            misses += int(not hit.any())
            if stored > vmax and hit.any():
                problems.append(f"{what}: a surface above every voxel")
            n += 2
    finally:
        r.close()
        t.close()
    FRAMES["iso"] = n
    assert not problems, f"{len(problems)} problems:\n" + "\n".join(problems[:40])
    assert hits >= 20 and misses >= 9, (hits, misses)


# ---------------------------------------------------------------------------------------------------------------
# item 5: reslice
# ---------------------------------------------------------------------------------------------------------------
def hip_reslice(r):
    r.render()
    return r.readPixels(), r.readResliceValues(), r.countSamples(per_pixel=True)[1]


def reslice_plane(vra, rng, dims, w, h, kind, n):
    """0: oblique, inside the volume; 1: oblique, partly outside; 2: an axis plane (partly outside: the image is wider than the volume)"""
    if kind == 2:
        axis = ("axial", "coronal", "sagittal")[int(rng.integers(3))]
        a = {"sagittal": 0, "coronal": 1, "axial": 2}[axis]
        return vra.axis_reslice(axis, int(rng.integers(dims[a])), dims, (1.0, 1.0, 1.0), (w, h), n=n, slab_step_mm=float(rng.choice([1.0, 0.25, 1.0 / 16.0])))
    centre = (np.array(dims, dtype=np.float64) - 1) / 2 + rng.uniform(-0.15, 0.15, size=3) * np.array(dims)
    pixel = (0.35 if kind == 0 else rng.uniform(1.0, 2.0)) * float(min(dims)) / float(max(w, h))
    step = float(rng.uniform(0.2, 2.0)) if n < 1000 else float(rng.uniform(0.02, 0.06))
    return vra.reslice_geometry(dims, (1.0, 1.0, 1.0), centre, rng.normal(size=3), rng.normal(size=3), pixel, step, (w, h))


@pytest.mark.parametrize("filt", [0, 1], ids=["nearest", "trilinear"])
def test_reslice_matrix(vra, oracle, rslib, filt):
    R = vra.renderer
    rng = np.random.default_rng(20261102 + filt)
    kinds = ("white", "scaled_rand", "scaled_ball", "white", "scaled_smooth")
    problems, with_nan, lit, n_frames = [], 0, 0, 0
    r, t = vra.RendererCore(0), vra.RendererCore(0)
    try:
        case = 0
        for mode in ("mip", "minip", "mean"):
            for n in (1, 3, 64, 1023, 1024):
                for plane in (0, 1, 2):
                    dims = tuple(int(v) for v in rng.integers(9, 48, size=3))
                    if case % 5 == 0:
                        dims = (dims[0] | 1, dims[1], dims[2])
                    w, h = (int(x) for x in rng.integers(17, 70 if n < 1000 else 41, size=2))      # (the long slabs on smaller frames: the reference's time)
                    v = u16.make(oracle, kinds[case % len(kinds)], dims, int(rng.integers(1 << 31)))
                    geom = reslice_plane(vra, rng, dims, w, h, plane, n)
                    layout = int(rng.integers(2))
                    use_tf = case % 2 == 1
                    quirk = case % 3 == 2                              # the +1000 on: window in, values out in stored - 1000
                    off = 1000 if quirk else 0
                    lo, hi = (int(rng.integers(0, 1300)) * 16, int(rng.integers(2000, 4096)) * 16) if case % 7 else (65535, 65535)
                    frames = []
                    for handle, vol, scale in ((r, v.vol, 1), (t, v.twin, v.scale)):
                        if vol is None:
                            continue
                        handle.setup((w, h))
                        assert handle.loadShader("VolumeRenderer.cs")
                        handle.setQuirks(R.QUIRK_U16_OFFSET if quirk and handle is r else 0)
                        handle.setLayout(layout)
                        handle.setVolume(vol)
                        handle.setFilter(filt)
                        handle.setWindow(lo // scale - (off if handle is r else 0), hi // scale - (off if handle is r else 0))
                        handle.setTransferFunction(TF_ISO, TF_RGBA) if use_tf else handle.setTransferFunction()
                        handle.setReslice(True, geom, mode=mode, n=n)
                        frames.append(hip_reslice(handle))
                        assert handle.last_kernel_name == RESLICE
                        handle.setReslice(False)
                    what = f"case {case}: {v.kind} {dims} {w}x{h} {mode} n {n} plane {plane} filt {filt} layout {layout} tf {use_tf} quirk {quirk} window [{lo}, {hi}]"
                    want = reslice_ref.render(rslib, v.vol, geom, w, h, mode=mode, n=n, filt=filt, min_val=lo, max_val=hi,
                                              tf_rgba=r.getTransferLut() if use_tf else None, u16_offset=quirk)
                    d = differ(frames[0], want)
                    if d:
                        problems.append(f"{what} vs reference: {d}")
                    nan = np.isnan(want[1])
                    with_nan += int(nan.any())
                    lit += int((want[2] > 0).sum())
                    if len(frames) == 2:
                        # the twin's picture and counts; its values exactly 16 times smaller (the +1000 taken back out where it was on)
                        d = differ((frames[0][0], frames[0][2]), (frames[1][0], frames[1][2]))
                        stored = frames[0][1] if not quirk else None
                        if stored is not None and not d:
                            d = differ((stored[~nan],), ((frames[1][1] * np.float32(v.scale))[~nan],))
                        if d:
                            problems.append(f"{what} vs the 12-bit twin: {d}")
                    n_frames += 1
                    case += 1
    finally:
        r.close()
        t.close()
    FRAMES[f"reslice[{filt}]"] = n_frames
    assert not problems, f"{len(problems)} problems:\n" + "\n".join(problems[:40])
    assert n_frames == 45 and with_nan >= 10 and lit > 1000, (n_frames, with_nan, lit)


def test_reslice_mean_of_1024_full_range_samples_is_summed_in_slab_order(vra, oracle, rslib):
    """the case of tests/test_u16_full_range_cpu.py in which the order of the fp32 sum shows in the bits: both layouts"""
    vol, geom, (w, h) = u16.mean_order_case(oracle)
    want = reslice_ref.render(rslib, vol, geom, w, h, mode="mean", n=1024, filt=0, min_val=0, max_val=65535, u16_offset=False)
    assert np.all(want[2] == 1024) and float(want[1].max()) * 1024 > 2.0 ** 24
    for layout in (0, 1):
        with vra.RendererCore(0) as r:
            r.setup((w, h))
            assert r.loadShader("VolumeRenderer.cs")
            r.setQuirks(0)
            r.setLayout(layout)
            r.setVolume(vol)
            r.setWindow(0, 65535)
            r.setReslice(True, geom, mode="mean", n=1024)
            got = hip_reslice(r)
            assert r.last_kernel_name == RESLICE
        assert not differ(got, want), (layout, differ(got, want))
    FRAMES["reslice_mean_order"] = 2


# ---------------------------------------------------------------------------------------------------------------
# item 6: shading
# ---------------------------------------------------------------------------------------------------------------
def hip_frame(r):
    r.render()
    return r.readPixels(), r.countSamples(per_pixel=True)[1]


def test_shading_matrix(vra, oracle, shadelib):
    rng = np.random.default_rng(20261103)
    poses = [dict(), dict(zenith=0.5, azimuth=0.8), dict(zenith=-0.7, azimuth=2.2), dict(zoom_in=3), dict(zoom_in=2, zenith=0.3, azimuth=-0.4),
             dict(zenith=1.2, azimuth=0.1)]
    kinds = ("scaled_ball", "white", "scaled_smooth", "scaled_rand")
    problems, lit, n = [], 0, 0
    r, t = vra.RendererCore(0), vra.RendererCore(0)
    try:
        for case in range(40):
            dims = tuple(int(v) for v in rng.integers(9, 48, size=3))
            if case % 5 == 0:
                dims = (dims[0] | 1, dims[1], dims[2])
            spacing = (1.0, 1.0, 1.0) if rng.integers(3) == 0 else tuple(float(v) for v in rng.uniform(0.5, 2.0, size=3).round(2))
            w, h = int(rng.integers(17, 70)), int(rng.integers(17, 70))
            v = u16.make(oracle, kinds[case % len(kinds)], dims, int(rng.integers(1 << 31)))
            view = VIEWS[int(rng.integers(3))]
            filt, layout, accum = case % 2, (case // 2) % 2, int(rng.integers(2))
            use_tf = (case // 4) % 2 == 1
            lo, hi = int(rng.integers(0, 1300)) * 16, int(rng.integers(2000, 4096)) * 16
            alpha = float(rng.choice([0.004, 0.05, 0.3, 1.0]))
            coef = COEFS[case % len(COEFS)]
            cam = orbit_cam(oracle, **poses[int(rng.integers(len(poses)))])
            frames = {}
            for handle, vol, scale in ((r, v.vol, 1), (t, v.twin, v.scale)):
                if vol is None:
                    continue
                handle.setup((w, h))
                assert handle.loadShader("VolumeRenderer.cs")
                handle.setQuirks(0)
                handle.setLayout(layout)
                handle.setVolume(vol, spacing)
                handle.setInitialCameraRotation(view == "top", view == "bottom")
                handle.setCameraBlock(cam)
                handle.setFilter(filt)
                handle.setAccum(accum)
                handle.setWindow(lo // scale, hi // scale)
                handle.setAlpha(alpha)
                handle.setMIP(False)
                handle.setTransferFunction(TF_ISO, TF_RGBA) if use_tf else handle.setTransferFunction()
                handle.setShading(True, *coef)
                for skip in ((False, True) if handle is r else (False,)):
                    handle.setSkipEmpty(skip)
                    frames[(handle is t, skip)] = hip_frame(handle)
                    assert handle.last_kernel_name == SHADE
                if handle is r and coef[:3] == (1.0, 0.0, 0.0):
                    handle.setShading(False)
                    frames["plain"] = hip_frame(handle)
                    assert handle.last_kernel_name != SHADE
            what = f"case {case}: {v.kind} {dims} {spacing} {w}x{h} {view} filt {filt} layout {layout} accum {accum} tf {use_tf} alpha {alpha} coef {coef}"
            p = oracle.OracleParams(w, h, cam=cam, voxel_size=spacing, alpha_scale=alpha, min_val=lo, max_val=hi, view_top=int(view == "top"),
                                    view_bottom=int(view == "bottom"), filter=filt, accum=accum, tf_rgba=r.getTransferLut() if use_tf else None)
            want = shade_ref.render(shadelib, v.vol, p, *coef)
            lit += int((want[0][..., 3] > 0).sum())
            for skip in (False, True):
                d = differ(frames[(False, skip)], want)
                if d:
                    problems.append(f"{what} skip {skip} vs reference: {d}")
            if "plain" in frames:
                d = differ(frames["plain"], want)
                if d:
                    problems.append(f"{what}: (1, 0, 0) is not the composite kernels' frame: {d}")
            if v.twin is not None:
                d = differ(frames[(False, False)], frames[(True, False)])
                if d:
                    problems.append(f"{what} vs the 12-bit twin: {d}")
            n += 2
    finally:
        r.close()
        t.close()
    FRAMES["shade"] = n
    assert not problems, f"{len(problems)} problems:\n" + "\n".join(problems[:40])
    assert lit > 1000, lit


# ---------------------------------------------------------------------------------------------------------------
# item 7: one handle whose value range changes
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", [0, 1], ids=["nearest", "trilinear"])
def test_one_handle_across_value_ranges(vra, oracle, filt):
    """12-bit, white, 12-bit again on one bricked handle with skipping and the packed copy on: a stale packed copy, apron copy,
    skip grid or exact range of the volume before would show in the frame"""
    R = vra.renderer
    dims, size = (45, 38, 41), (96, 80)
    low = oracle.gen_noise_ball(dims, 2, 77)
    white = u16.make(oracle, "white", dims, 78).vol
    low2 = u16.smooth12(np.random.default_rng(79), dims)
    cam = orbit_cam(oracle, 0.42, 0.54)
    n = 0
    with vra.RendererCore(0) as r:
        r.setup(size)
        assert r.loadShader("VolumeRenderer.cs")
        r.setQuirks(0); r.setLayout(R.LAYOUT_BRICKED); r.setPack12(1); r.setSkipEmpty(True)
        r.setFilter(filt); r.setAlpha(0.3)
        for step, (vol, win) in enumerate(((low, (64, 4095)), (white, (20000, 60000)), (low, (64, 4095)), (white, (64, 4095)), (low2, (1500, 3900)))):
            r.setVolume(vol)
            assert r.dataset_range == (int(vol.min()), int(vol.max())) and r.window == r.dataset_range
            r.setWindow(*win)
            r.setCameraBlock(cam)                                 # (loading a volume resets the camera, as the reference does)
            for variant in ((0, 3) if filt == 0 else (0, 6)):
                r.setKernelVariant(variant)
                r.render()
                got = (r.readPixels(), r.countSamples(per_pixel=True)[1])
                name = r.last_kernel_name
                packs = int(vol.max()) <= 4095
                if filt == 0:
                    assert name in FASTS and (r.pack12Bytes() > 0) == packs, (step, variant, name, r.pack12Bytes())
                else:
                    assert name in (TSLAB, TRI) and r.pack12Bytes() == 0 and r.trilinearCopyBytes() > 0, (step, variant, name)
                p = oracle.OracleParams(size[0], size[1], cam=cam, alpha_scale=0.3, min_val=win[0], max_val=win[1], filter=filt)
                want, _, want_spp = oracle.render(vol, p, want_spp=True)
                assert not differ(got, (want, want_spp)), (step, variant, name, differ(got, (want, want_spp)))
                assert (want[..., 3] > 0).sum() > 280
                n += int(not packs)
    FRAMES[f"one_handle[{filt}]"] = n


# ---------------------------------------------------------------------------------------------------------------
# item 8: shards
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tf", [False, True], ids=["grey", "tf"])
def test_stripes_and_a_group_assemble_the_full_range_frame(vra, oracle, tf):
    v = u16.make(oracle, "white" if tf else "scaled_ball", (48, 40, 44), 88)
    size = (133, 101)
    w, h = size
    win = (20000, 48671) if tf else (1024, 65520)
    cam = orbit_cam(oracle, 0.3, -0.5)

    def configure(m):
        assert m.loadShader("VolumeRenderer.cs")
        m.setQuirks(0)
        m.setVolume(v.vol)
        m.setWindow(*win)
        m.setAlpha(0.05)
        m.setCameraBlock(cam)
        if tf:
            m.setTransferFunction(*TF_KNOTS)

    with vra.RendererCore(0) as r:
        r.setup(size)
        configure(r)
        r.render()
        full = r.readPixels()
        p = oracle.OracleParams(w, h, cam=cam, alpha_scale=0.05, min_val=win[0], max_val=win[1], tf_rgba=r.getTransferLut() if tf else None)
        want, _ = oracle.render(v.vol, p)
        assert np.array_equal(bits(full), bits(want)) and (full[..., 3] > 0).sum() > 1000
        acc = np.zeros_like(full)
        for k in range(3):                                    # cyclic stripes of 8 rows, three ways, on the own full-size target
            r.setRowStripes(8, k, 3)
            r.render()
            rows = np.array([y for y in range(h) if (y // 8) % 3 == k])
            acc[rows] = r.readPixels()[rows]
        r.setRowStripes(1, 0, 1)
        assert np.array_equal(bits(acc), bits(full))
    with vra.RendererGroup([0, 0, 0]) as g:                   # compact (grey, alpha) or RGBA shard targets, gathered and assembled
        g.setup(size, partition="stripes", stripe_rows=16)
        g.each(configure)
        g.render()
        assert np.array_equal(bits(g.readPixels()), bits(full))
    FRAMES[f"shards[{tf}]"] = 3


# ---------------------------------------------------------------------------------------------------------------
# item 9: the 16-bit histogram and the dataset range
# ---------------------------------------------------------------------------------------------------------------
def reference_histogram(vol):
    """RendererCore.cpp:386-405 of the reference for 16-bit data, operation by operation in float32"""
    f32 = np.float32
    vmax = int(vol.max())
    x = (vol.astype(f32).ravel() * f32(255.0)).astype(f32) / f32(vmax)
    b = np.floor(x.astype(np.float64) + 0.5).astype(np.int64) & 0xFFFF      # std::round of a value >= 0; stored to uint16_t
    counts = np.bincount(b[(b != 0) & (b < 256)], minlength=256)
    norm = max(vmax, int(counts.max()))                       # starts at the dataset maximum, raised to the largest count
    return (counts.astype(f32) * f32(100.0) / f32(norm)).astype(f32), norm > vmax


@pytest.mark.parametrize("vmax", [300, 4095, 65535])
@pytest.mark.parametrize("layout", [0, 1], ids=["linear", "bricked"])
def test_u16_histogram_and_dataset_range(vra, oracle, vmax, layout):
    rng = np.random.default_rng(vmax + layout)
    dims = (45, 38, 41)
    raised = 0
    for flavour in ("uniform", "peaked"):
        vol = rng.integers(0, vmax + 1, size=dims[::-1]).astype(np.uint16)
        if flavour == "peaked":                                # most voxels in one bin: its count passes the dataset maximum (vmax = 300, 4095)
            vol[rng.random(size=vol.shape) < 0.6] = vmax // 2
        vol.flat[5], vol.flat[-7] = vmax, 3
        with vra.RendererCore(0) as r:
            r.setup((32, 32))
            assert r.loadShader("VolumeRenderer.cs")
            r.setLayout(layout)
            r.setVolume(vol)
            assert r.dataset_range == (int(vol.min()), int(vol.max())) == r.window
            got = r.histogram()
        want, was_raised = reference_histogram(vol)
        raised += int(was_raised)
        assert got[0] == 0.0 and want[1:].any()
        assert np.allclose(got, want, rtol=1e-6, atol=0), (flavour, np.argwhere(got != want)[:5].ravel(), got[got != want][:5], want[got != want][:5])
    assert raised >= (1 if vmax <= 4095 else 0)


# ---------------------------------------------------------------------------------------------------------------
# every kernel the library can name, on full-range data, in one place
# ---------------------------------------------------------------------------------------------------------------
def test_every_kernel_name_appears_on_full_range_data(vra, oracle, isolib, rslib, shadelib):
    R = vra.renderer
    dims, size = (45, 38, 41), (96, 80)
    v = u16.make(oracle, "white", dims, 99)
    cam = orbit_cam(oracle, 0.42, 0.54)
    seen = {}
    with Scene(vra, oracle, v.vol, size) as s:
        for variant, filt, accum in ((2, 0, 0), (3, 0, 0), (1, 0, 0), (2, 1, 0), (6, 1, 0)):
            kw = dict(win=(9000, 60000), alpha=0.3, cam=cam, variant=variant, filt=filt, accum=accum)
            got, name = s.frame(**kw)
            assert not differ(got, s.want(**kw)), (name, differ(got, s.want(**kw)))
            seen[name] = seen.get(name, 0) + 1
        r = s.r
        r.setKernelVariant(0)
        p = oracle.OracleParams(size[0], size[1], cam=cam, alpha_scale=0.3, min_val=9000, max_val=60000, filter=1)
        r.setIsosurface(True, 50000)
        got = hip_iso(r)
        seen[r.last_kernel_name] = 1
        assert not differ(got, iso_ref.render(isolib, v.vol, p, 50000, u16_offset=False)) and np.isfinite(got[1]).any()
        r.setIsosurface(False, 0)
        geom = vra.reslice_geometry(dims, (1, 1, 1), (22.0, 18.0, 20.0), (0.3, 0.4, 1.0), (0.0, 1.0, 0.0), 0.6, 0.8, size)
        r.setReslice(True, geom, mode="minip", n=7)
        got = hip_reslice(r)
        seen[r.last_kernel_name] = 1
        assert not differ(got, reslice_ref.render(rslib, v.vol, geom, size[0], size[1], mode="minip", n=7, filt=1, min_val=9000, max_val=60000, u16_offset=False))
        r.setReslice(False)
        r.setShading(True, *COEFS[0])
        got = hip_frame(r)
        seen[r.last_kernel_name] = 1
        assert not differ(got, shade_ref.render(shadelib, v.vol, p, *COEFS[0]))
        assert r.pack12Bytes() == 0
    FRAMES["every_kernel"] = 8
    assert set(seen) == {FAST, RELAY, GENERIC, TRI, TSLAB, ISO, RESLICE, SHADE}, seen
