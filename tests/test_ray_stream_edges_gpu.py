"""The ray-ordered sample stream (csrc/vr_stream.hip) at its edges, against the CPU oracle.

tests/test_ray_stream_gpu.py compares a replayed frame with the same handle's gather-kernel frame, at three image sizes that are
multiples of 8, cubic spacing and setQuirks(0).  Here every replayed frame is compared bit for bit with oracle.render first, then
with the gather frame (which tells a fault of the stream from a shared one), and `raymarch_stream_kernel` is asserted on every
one of them.  The cases are tests/ray_stream_cases.py's; tests/test_ray_stream_cases_cpu.py proves on the CPU that each reaches
the branch it is for.

B1  the scan with 2, 3 and 5 blocks per thread, idle threads and a cut-short one (images of 1496 to 4408 stream blocks)
B2  stream blocks cut by the image edge (101x77, 97x65, 8x8), with and without kQuirkTruncGrid, a row range, cyclic stripes
B3  the 64-bit record instances: both sides of the bricked and the linear stride threshold of tests/offset_limits.py
B4  rays that end at the step cap of 10000 samples
B5  rays that end at every position inside a group of four, by opacity and by geometry; constant volumes that end every ray at
    sample 11 (= 4 * 2 + 3) and 12
B6  the stream's size, to the byte, from the oracle's geometric sample counts
B7  the default quirks (the 16-bit window offset), anisotropic spacing, an eye inside the box
B8  a stream refused for its size is refused for that geometry only

What catches what (checked once by hand on copies of the library, nothing of them kept) is in docs/lab-notebook.md, "Ray stream
edges".  Not here: a stream of more than 2^32 elements, and bench.py's --extras orbit entry.
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


S = _load("ray_stream_cases", _HERE / "ray_stream_cases.py")
E = _load("edge_cases", _HERE / "edge_cases.py")
O = _load("offset_limits", _HERE / "offset_limits.py")

STREAM = S.STREAM
KINDS = pytest.mark.parametrize("kind", ["u8", "u16"])
WINDOWS = {"u8": [(0, 255), (20, 200)], "u16": [(0, 4095), (500, 3000)]}      # the data's whole range (no clamp) and a clamp on both sides


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(bits(got), bits(want)):
        bad = np.argwhere(bits(got) != bits(want))
        raise AssertionError(f"{what}: {len(bad)} words differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}")


def fresh(vra, size, vol=None, spacing=(1.0, 1.0, 1.0), quirks=0, layout=None):
    """quirks=None: the handle keeps VR_QUIRK_DEFAULT, like a caller who sets nothing"""
    R = vra.renderer
    r = vra.RendererCore(0)
    r.setup(size)
    assert r.loadShader("VolumeRenderer.cs")
    if quirks is not None:
        r.setQuirks(quirks)
    r.setLayout(R.LAYOUT_BRICKED if layout is None else layout)
    if vol is not None:
        r.setVolume(vol, spacing)
    return r


def set_mode(r, mode):
    """the transfer function's table for the oracle, or None"""
    r.setMIP(mode in ("mip", "mip_tf"))
    if mode in ("tf", "mip_tf"):
        r.setTransferFunction(S.TF_ISO, S.TF_COLOUR)
    elif mode == "grey_tf":
        r.setTransferFunction(S.TF_ISO, S.TF_GREY)
    else:
        r.setTransferFunction()
        return None
    return r.getTransferLut()


def replayed_and_gathered(r, what):
    """the frame at mode 2 and the same handle's frame at mode 0; asserts which kernels ran"""
    r.setRayStream(2)
    r.render()
    assert r.last_kernel_name == STREAM, (what, r.last_kernel_name)
    a = r.readPixels().copy()
    r.setRayStream(0)
    r.render()
    assert r.last_kernel_name != STREAM, what
    return a, r.readPixels().copy()


def check(r, oracle, vol, p, what, rows=None, trunc=False):
    """The replayed frame of the handle's state against the oracle's frame for `p` -- on the launch's own pixels: `rows` (image
    rows, -1: none; default all) left of kQuirkTruncGrid's limit -- and then, whole, against the gather kernels' frame: what a
    launch does not write must hold the same either way.  Returns the replayed frame."""
    a, b = replayed_and_gathered(r, what)
    want = oracle.render(vol, p)[0]
    h, w = want.shape[:2]
    own = [py for py in (range(h) if rows is None else rows) if py >= 0]
    if trunc:
        own = [py for py in own if py < h // S.LOCAL_SIZE * S.LOCAL_SIZE]
    cols = w // S.LOCAL_SIZE * S.LOCAL_SIZE if trunc else w
    assert_same(a[own, :cols], want[own, :cols], what + ": replayed frame against the oracle")
    assert_same(a, b, what + ": replayed frame against the gather kernels' frame")
    return a


def model_bytes(oracle, vol, size, cam, spacing=(1.0, 1.0, 1.0), rows=None, trunc=False):
    n = S.geometric_counts(oracle, vol, size, cam, spacing=spacing, window=(0, 255))
    return S.stream_bytes(S.local_counts(n, S.local_rows(size[1], trunc=trunc) if rows is None else rows, trunc), vol.dtype.itemsize)


def pose_camera(r, pose):
    r.resetCamera()
    for call in pose:
        r.cameraOrient(*call)
    return r.getCameraBlock()


# ---------------------------------------------------------------------------------------------------------------
# B1: the scan
# ---------------------------------------------------------------------------------------------------------------
@KINDS
@pytest.mark.parametrize("size", list(S.SCAN_SIZES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_scan_with_several_blocks_per_thread(vra, oracle, size, kind):
    """grey composite of the 64^3 noise ball at images of 1024 (the boundary), 1496, 2312 and 4408 stream blocks: the default
    camera (blocks of one length, and empty ones) and a pose that looks at an edge (blocks of many lengths).  The first build's
    size is the model's: an offset table that is wrong past its first 1024 entries shows in the frame or in the total"""
    blocks, per, _, _ = S.SCAN_SIZES[size]
    assert S.stream_grid(*size).blocks == blocks and S.scan_shape(blocks).per == per
    vol = S.residue_volume(oracle, kind)
    win = S.residue_window(kind)
    with fresh(vra, size, vol) as r:
        r.setWindow(*win); r.setAlpha(S.SCAN_ALPHA)
        for k, pose in enumerate(S.RESIDUE_POSES):
            cam = pose_camera(r, pose)
            what = f"{size} {kind} pose {pose}"
            a = check(r, oracle, vol, S.params(oracle, size, cam, S.SCAN_ALPHA, win), what)
            assert np.count_nonzero(a[..., 3]) >= 1000, what
            if k == 0:
                r.setRayStream(2)
                r.render()
                assert r.rayStreamBytes() == model_bytes(oracle, vol, size, cam), what
        assert r.rayStreamBuilds() == len(S.RESIDUE_POSES)


# ---------------------------------------------------------------------------------------------------------------
# B2: blocks cut by the image edge
# ---------------------------------------------------------------------------------------------------------------
@KINDS
@pytest.mark.parametrize("trunc", [False, True], ids=["whole", "trunc_grid"])
@pytest.mark.parametrize("size", S.PARTIAL_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_blocks_cut_by_the_image_edge(vra, oracle, size, trunc, kind):
    """every mode x pose x alpha x window at 101x77, 97x65 and 8x8; with kQuirkTruncGrid the launch ends at 96x64 (0x0 for 8x8:
    a stream without a sample) and the pixels beyond hold what the gather kernels leave there.  From the close pose every lane
    inside the image has samples; the size after each pose's first build is the model's (of the longest so far): lanes
    outside the image hold no sample"""
    vol = S.residue_volume(oracle, kind)
    lit, models = 0, []
    with fresh(vra, size, vol, quirks=vra.renderer.QUIRK_TRUNC_GRID if trunc else 0) as r:
        for mode in S.MODES:
            lut = set_mode(r, mode)
            for pose in S.PARTIAL_POSES:
                cam = pose_camera(r, pose)
                for alpha in (0.004, 1.0):
                    r.setAlpha(alpha)
                    for win in WINDOWS[kind]:
                        r.setWindow(*win)
                        what = f"{size} trunc {trunc} {kind} {mode} pose {pose} alpha {alpha} window {win}"
                        first = mode == S.MODES[0] and alpha == 0.004 and win == WINDOWS[kind][0]     # the first build of this pose
                        a = check(r, oracle, vol, S.params(oracle, size, cam, alpha, win, mode, lut, trunc=trunc), what, trunc=trunc)
                        lit += int(np.count_nonzero(a[..., 3]) > 0)
                        if first:
                            r.setRayStream(2)
                            r.render()
                            # (the sample buffer is kept where it is large enough: the longest stream so far)
                            models.append(model_bytes(oracle, vol, size, cam, trunc=trunc))
                            assert r.rayStreamBytes() == max(models), (what, models)
    assert (lit == 0) if (trunc and size == (8, 8)) else (lit >= 45)                # of 60 frames


@KINDS
@pytest.mark.parametrize("trunc", [False, True], ids=["whole", "trunc_grid"])
def test_row_range_and_stripes_inside_blocks(vra, oracle, trunc, kind):
    """101x77: rows 13..58 (the range begins and ends inside a block) and rank 1 of 3 in cyclic stripes of 16 rows (rows 16..31
    and 64..76: the image cuts the second stripe, kQuirkTruncGrid removes it)"""
    size = (101, 77)
    vol = S.residue_volume(oracle, kind)
    win = WINDOWS[kind][1]
    with fresh(vra, size, vol, quirks=vra.renderer.QUIRK_TRUNC_GRID if trunc else 0) as r:
        r.setWindow(*win)
        for mode in ("grey", "mip", "tf"):
            lut = set_mode(r, mode)
            for pose in S.PARTIAL_POSES:
                cam = pose_camera(r, pose)
                for alpha in (0.004, 1.0):
                    r.setAlpha(alpha)
                    what = f"trunc {trunc} {kind} {mode} pose {pose} alpha {alpha}"
                    r.setRowRange(*S.PARTIAL_ROW_RANGE)
                    rows = S.local_rows(size[1], row_range=S.PARTIAL_ROW_RANGE, trunc=trunc)
                    assert r.localRows() == len(rows)
                    p = S.params(oracle, size, cam, alpha, win, mode, lut, trunc=trunc, row_range=S.PARTIAL_ROW_RANGE)
                    a = check(r, oracle, vol, p, what + " row range", rows=rows, trunc=trunc)
                    assert np.count_nonzero(a[rows[0]:rows[-1] + 1, :, 3]) > 0
                    r.setRowRange(0, -1)
                    r.setRowStripes(*S.PARTIAL_STRIPES)
                    rows = S.local_rows(size[1], stripes=S.PARTIAL_STRIPES, trunc=trunc)
                    assert r.localRows() == len(rows)
                    p = S.params(oracle, size, cam, alpha, win, mode, lut, trunc=trunc)       # rows picked out of a full frame
                    check(r, oracle, vol, p, what + " stripes", rows=rows, trunc=trunc)
                    r.setRowStripes(1, 0, 1)


# ---------------------------------------------------------------------------------------------------------------
# B3: the 64-bit record instances
# ---------------------------------------------------------------------------------------------------------------
OFFSET_SIZE = (96, 64)
OFFSET_ALPHA = 0.001
OFFSET_WINDOW = {1: (10, 200), 2: (1500, 2500)}
_volumes = {}


def threshold_volume(dims, dtype):
    """random voxels; the last one drawn is kept for the next test (tests/test_offset_limits_gpu.py)"""
    key = (dims, np.dtype(dtype).name)
    if key not in _volumes:
        _volumes.clear()
        _volumes[key] = O.rand_voxels(np.random.default_rng(sum(dims) + np.dtype(dtype).itemsize), dims, dtype)
    return _volumes[key]


def reads_the_last_voxel(render_ref, vol):
    """the reference's frame with the last voxel at its largest and at its smallest value differ: a sample of the frame reads
    voxel (nx - 1, ny - 1, nz - 1), where every factor of the address is largest.  The volume is restored."""
    keep = vol.flat[-1]
    frames = []
    for value in (E.vmax_of(vol.dtype), 0):
        vol.flat[-1] = value
        frames.append(render_ref())
    vol.flat[-1] = keep
    return not np.array_equal(bits(frames[0]), bits(frames[1]))


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
@pytest.mark.parametrize("side", ["inside", "outside"], ids=["32bit", "64bit"])
@pytest.mark.parametrize("name", ["bstride_z", "ny*nz"])
def test_record_kernel_on_both_sides_of_a_stride_threshold(vra, oracle, name, side, dtype):
    """stream_record_kernel<VoxelT, LAYOUT, BIG> for both voxel types, both layouts and both values of BIG: volumes of 32 to 128
    MiB on either side of the 24-bit stride limit, from the corner camera (its frame reads the last voxel) and an orbit pose, as
    grey composite and MIP"""
    t = O.THRESHOLDS[name]
    dims = getattr(t, side)
    b = np.dtype(dtype).itemsize
    assert O.takes_32bit_path(dims, b, t.layout) == (side == "inside")
    vol = threshold_volume(dims, dtype)
    lo, hi = OFFSET_WINDOW[b]
    orbit = oracle.Camera()
    orbit.orient(0.0, -0.3, 0.5)
    with fresh(vra, OFFSET_SIZE, vol, t.spacing, layout=t.layout) as r:
        r.setWindow(lo, hi); r.setAlpha(OFFSET_ALPHA)
        for cname, block in (("corner", O.corner_camera(E, dims, t.spacing, "front")), ("orbit", orbit.block())):
            r.setCameraBlock(block)
            for mode in ("grey", "mip"):
                set_mode(r, mode)
                p = S.params(oracle, OFFSET_SIZE, block, OFFSET_ALPHA, (lo, hi), mode, spacing=t.spacing, threads=8)
                what = f"{name} {side} {dims} {np.dtype(dtype).name} {cname} {mode}"
                if cname == "corner" and mode == "grey":
                    assert reads_the_last_voxel(lambda: oracle.render(vol, p)[0], vol), what
                a = check(r, oracle, vol, p, what)
                assert np.count_nonzero(a[..., 3]) > 0, what
                assert r.pack12Bytes() == 0, what


# ---------------------------------------------------------------------------------------------------------------
# B4: the step cap
# ---------------------------------------------------------------------------------------------------------------
def test_rays_that_end_at_the_step_cap(vra, oracle):
    """16384 x 4 x 4 voxels seen down the long axis: 484 rays stop at 10000 samples with dest.a <= 0.40 (the CPU file), a
    stream block of 2500 groups beside blocks of a few"""
    vol = S.cap_volume()
    cam = S.cap_camera()
    with fresh(vra, S.CAP_SIZE, vol, S.CAP_SPACING) as r:
        r.setWindow(*S.CAP_WINDOW); r.setAlpha(S.CAP_ALPHA)
        r.setCameraBlock(cam)
        for mode in ("grey", "mip"):
            set_mode(r, mode)
            p = S.params(oracle, S.CAP_SIZE, cam, S.CAP_ALPHA, S.CAP_WINDOW, mode, spacing=S.CAP_SPACING)
            check(r, oracle, vol, p, f"step cap {mode}")
        r.setRayStream(0)
        _, spp = r.countSamples(per_pixel=True)
        assert np.count_nonzero(spp == S.MAX_STEPS) >= 100 and spp.max() == S.MAX_STEPS
        r.setRayStream(2)
        r.render()
        assert r.last_kernel_name == STREAM
        assert r.rayStreamBytes() == model_bytes(oracle, vol, S.CAP_SIZE, cam, spacing=S.CAP_SPACING)


# ---------------------------------------------------------------------------------------------------------------
# B5: where a ray ends inside a group of four
# ---------------------------------------------------------------------------------------------------------------
@KINDS
def test_rays_end_at_every_position_of_a_group(vra, oracle, kind):
    """the frames whose rays the CPU file counts per residue: the noise ball from the default camera and from the edge pose at
    alpha 1.0, 0.3 and 0.004, as grey composite, MIP and through a colour transfer function"""
    vol = S.residue_volume(oracle, kind)
    win = S.residue_window(kind)
    with fresh(vra, S.RESIDUE_SIZE, vol) as r:
        r.setWindow(*win)
        for pose in S.RESIDUE_POSES:
            cam = pose_camera(r, pose)
            for mode in ("grey", "mip", "tf"):
                lut = set_mode(r, mode)
                for alpha in S.RESIDUE_ALPHAS:
                    r.setAlpha(alpha)
                    check(r, oracle, vol, S.params(oracle, S.RESIDUE_SIZE, cam, alpha, win, mode, lut), f"{kind} pose {pose} {mode} alpha {alpha}")
        assert r.rayStreamBuilds() >= len(S.RESIDUE_POSES)


@KINDS
@pytest.mark.parametrize("value,alpha,count", S.CONSTANT_CASES)
def test_constant_volume_ends_every_ray_at_one_sample(vra, oracle, kind, value, alpha, count):
    """every long ray stops after `count` samples: 11 -- the last sample of the third group is the first one left out, the
    whole-group shortcut's own test decides -- and 12"""
    vol = S.constant_volume(value, kind)
    with fresh(vra, S.RESIDUE_SIZE, vol) as r:
        r.setWindow(0, 255); r.setAlpha(alpha)
        cam = pose_camera(r, ())
        for mode in ("grey", "grey_tf", "tf"):
            lut = set_mode(r, mode)
            check(r, oracle, vol, S.params(oracle, S.RESIDUE_SIZE, cam, alpha, (0, 255), mode, lut), f"constant {value} {kind} alpha {alpha} {mode}")
        set_mode(r, "grey")
        _, spp = r.countSamples(per_pixel=True)
        assert np.count_nonzero(spp == count) >= 1000 and spp.max() == count


# ---------------------------------------------------------------------------------------------------------------
# B6: the stream's size
# ---------------------------------------------------------------------------------------------------------------
@KINDS
@pytest.mark.parametrize("pose", S.PARTIAL_POSES, ids=["default", "edge", "close"])
@pytest.mark.parametrize("size,row_range", S.BYTES_CASES, ids=lambda v: "x".join(map(str, v)) if v else "all")
def test_stream_size_to_the_byte(vra, oracle, size, row_range, pose, kind):
    """a fresh handle, one forced build: sum over blocks of ceil(max n / 4) * 256 voxels + 16 bytes, 128 bytes of counts per
    block and blocks + 1 offsets of 8, n from the oracle at alpha_scale = 0"""
    vol = S.residue_volume(oracle, kind)
    win = S.residue_window(kind)
    with fresh(vra, size, vol) as r:
        r.setWindow(*win); r.setAlpha(0.05)
        cam = pose_camera(r, pose)
        if row_range is not None:
            r.setRowRange(*row_range)
        r.setRayStream(2)
        r.render()
        assert r.last_kernel_name == STREAM and r.rayStreamBuilds() == 1
        rows = S.local_rows(size[1], row_range=row_range)
        assert r.rayStreamBytes() == model_bytes(oracle, vol, size, cam, rows=rows), (size, row_range, pose, kind)
        assert r.rayStreamBytes() > 16 + S.stream_grid(size[0], len(rows)).blocks * 136 + 8      # (there are samples)


# ---------------------------------------------------------------------------------------------------------------
# B7: quirks, spacing, an eye inside the box
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quirks", [None, 2, 3], ids=["default", "u16_offset", "u16_offset+trunc_grid"])
def test_the_u16_window_offset(vra, oracle, quirks):
    """16-bit data under VR_QUIRK_U16_OFFSET -- what a caller who sets nothing gets -- alone and with kQuirkTruncGrid: the
    caller's window (-500, 2000) is the oracle's (500, 3000); window, MIP and a colour transfer function (2501 entries of the
    classification table)"""
    R = vra.renderer
    assert R.QUIRK_DEFAULT == R.QUIRK_U16_OFFSET == 2
    size = (101, 77)
    trunc = quirks == 3
    vol = S.residue_volume(oracle, "u16")
    with fresh(vra, size, vol, quirks=quirks) as r:
        for lo, hi in ((-500, 2000), (-1000, 3095)):
            r.setWindow(lo, hi)
            win = (lo + 1000, hi + 1000)
            for pose in S.RESIDUE_POSES:
                cam = pose_camera(r, pose)
                for mode in ("grey", "mip", "tf"):
                    lut = set_mode(r, mode)
                    for alpha in (0.02, 1.0):
                        r.setAlpha(alpha)
                        what = f"quirks {quirks} window {(lo, hi)} pose {pose} {mode} alpha {alpha}"
                        a = check(r, oracle, vol, S.params(oracle, size, cam, alpha, win, mode, lut, trunc=trunc), what, trunc=trunc)
                        assert np.count_nonzero(a[..., 3]) >= 100, what


@KINDS
def test_anisotropic_spacing_and_an_eye_inside(vra, oracle, kind):
    """40 x 56 x 24 voxels of 1.0 x 0.8 x 1.7 (three extents, the certified division) from the orbit poses of
    tests/test_parity_gpu.py and from a camera block whose eye lies inside the box (t_min clamped at the eye); front and top view"""
    vol = S.aniso_volume(kind)
    size = S.ANISO_SIZE
    win = (10, 200) if kind == "u8" else (100, 3000)
    with fresh(vra, size, vol, S.ANISO_SPACING) as r:
        r.setWindow(*win)
        for view in ("front", "top"):
            r.setInitialCameraRotation(rotate_to_top=view == "top", rotate_to_bottom=False)
            for name, cam in S.orbit_blocks(oracle) + [("inside", S.inside_camera())]:
                r.setCameraBlock(cam)
                for mode in ("grey", "mip"):
                    set_mode(r, mode)
                    for alpha in (1.0, 0.05):
                        r.setAlpha(alpha)
                        p = S.params(oracle, size, cam, alpha, win, mode, spacing=S.ANISO_SPACING, view=view)
                        a = check(r, oracle, vol, p, f"{kind} {view} {name} {mode} alpha {alpha}")
                        assert np.count_nonzero(a[..., 3]) >= 100


# ---------------------------------------------------------------------------------------------------------------
# B8: a refusal holds for one geometry
# ---------------------------------------------------------------------------------------------------------------
@KINDS
def test_a_refused_stream_is_refused_for_its_geometry_only(vra, oracle, kind):
    """The stream's size depends on the view.  Under a budget that holds the far view's stream and not the close view's, the
    close view is refused (and not asked again while it stands), the far view replays, the close view is refused again."""
    vol = S.residue_volume(oracle, kind)
    win = S.residue_window(kind)
    size = S.REFUSAL_SIZE
    alpha = 0.02
    cam_a, cam_b = S.refusal_cameras(oracle)

    def view(r, which):
        r.resetCamera()
        if which == "B":
            for _ in range(S.REFUSAL_DOLLY_STEPS):
                r.cameraOrient(-1.0, 0.0, 0.0)
        assert np.array_equal(bits(r.getCameraBlock()), bits(cam_b if which == "B" else cam_a))

    want = {w: oracle.render(vol, S.params(oracle, size, c, alpha, win))[0] for w, c in (("A", cam_a), ("B", cam_b))}
    nbytes = {}
    with fresh(vra, size, vol) as r:                                   # the automatic budget: both are built
        r.setWindow(*win); r.setAlpha(alpha)
        r.setRayStream(2)
        for which, cam in (("A", cam_a), ("B", cam_b)):
            view(r, which)
            r.render()
            assert r.last_kernel_name == STREAM
            assert_same(r.readPixels(), want[which], f"view {which} under the automatic budget")
            nbytes[which] = r.rayStreamBytes()
        assert nbytes["A"] == model_bytes(oracle, vol, size, cam_a)    # (B's allocation is A's, kept: no model for it here)
    with fresh(vra, size, vol) as r:
        r.setWindow(*win); r.setAlpha(alpha)
        view(r, "B")
        r.setRayStream(2)
        r.render()
        nbytes["B"] = r.rayStreamBytes()
        assert nbytes["B"] == model_bytes(oracle, vol, size, cam_b)
    assert nbytes["A"] >= 2 * nbytes["B"], nbytes
    with fresh(vra, size, vol) as r:
        r.setWindow(*win); r.setAlpha(alpha)
        r.setRayStream(0)
        view(r, "A")
        r.render()
        copies = r.residentBytes()[1]
        r.setCopyBudget(copies + nbytes["B"] + 4096)
        r.setRayStream(2)
        for _ in range(2):                                             # a refusal is remembered for the geometry it was given for
            r.render()
            assert r.last_kernel_name != STREAM
            assert_same(r.readPixels(), want["A"], "view A, refused")
        assert r.rayStreamBytes() == 0 and r.rayStreamBuilds() == 0
        view(r, "B")
        r.render()
        assert r.last_kernel_name == STREAM, "the far view's stream fits the budget: the close view's refusal must not outlive the close view"
        assert_same(r.readPixels(), want["B"], "view B, replayed")
        assert r.rayStreamBytes() == nbytes["B"] and r.rayStreamBuilds() == 1
        assert r.residentBytes()[1] == copies + nbytes["B"]
        view(r, "A")
        for _ in range(2):
            r.render()
            assert r.last_kernel_name != STREAM
            assert_same(r.readPixels(), want["A"], "view A, refused again")
        assert r.rayStreamBytes() == 0 and r.rayStreamBuilds() == 1
        assert r.residentBytes()[1] <= copies + nbytes["B"] + 4096
