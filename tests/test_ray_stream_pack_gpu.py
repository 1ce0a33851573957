"""The 12-bit packed format of the ray-ordered sample stream (vr_set_ray_stream_pack; csrc/vr_stream.hip, vr_stream_pack.h).

Every replayed frame is compared bit for bit with oracle.render first, then with the same handle's gather-kernel frame, and
`raymarch_stream12_kernel` is asserted on each of them (mode 2: pack whenever the volume allows; the automatic mode packs no
stream as small as a test's).  Geometry, cameras and modes are tests/ray_stream_cases.py's, the packed cases
tests/ray_stream_pack_cases.py's; tests/test_ray_stream_pack_cpu.py proves on the CPU that each reaches what it is for.

P1  rays that end at each of the eight positions of a group: by their length (the edge pose) and by the 0.95 test (constant
    volumes that end every long ray after 8 .. 15 samples)
P2  voxels of alternating 0x000 / 0xFFF / 0x555 / 0xAAA
P3  a volume offset by 1000 (range [1000, 5095]) under windows that contain its range, cut into it from either side and lie
    wholly below the base; a window too wide for the shifted constants
P4  every mode on every volume: grey, MIP, transfer function, its grey fold, MIP with a transfer function
P5  a span of 4096 and an 8-bit volume keep the old format: its size to the byte, its kernel name
P6  the packed stream's size to the byte; stripes and a row range that begin and end inside blocks
P7  a 64-bit-offset volume; several blocks per scan thread
P8  switching the pack mode on a live handle; the copy budget at the packed size
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


C = _load("ray_stream_pack_cases", _HERE / "ray_stream_pack_cases.py")
S = C.S
E = _load("edge_cases", _HERE / "edge_cases.py")
O = _load("offset_limits", _HERE / "offset_limits.py")

STREAM, STREAM12 = S.STREAM, C.STREAM12


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(bits(got), bits(want)):
        bad = np.argwhere(bits(got) != bits(want))
        raise AssertionError(f"{what}: {len(bad)} words differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}")


def fresh(vra, size, vol, spacing=(1.0, 1.0, 1.0), layout=None, pack=2):
    R = vra.renderer
    r = vra.RendererCore(0)
    r.setup(size)
    assert r.loadShader("VolumeRenderer.cs")
    r.setQuirks(0)
    r.setLayout(R.LAYOUT_BRICKED if layout is None else layout)
    r.setVolume(vol, spacing)
    assert r.rayStreamPack() == 1                  # the default: automatic
    r.setRayStreamPack(pack)
    assert r.rayStreamPack() == pack
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


def pose_camera(r, pose):
    r.resetCamera()
    for call in pose:
        r.cameraOrient(*call)
    return r.getCameraBlock()


def check(r, oracle, vol, p, what, rows=None, kernel=STREAM12):
    """the replayed frame against the oracle's on the launch's own rows, then whole against the gather kernels' frame"""
    r.setRayStream(2)
    r.render()
    assert r.last_kernel_name == kernel, (what, r.last_kernel_name)
    a = r.readPixels().copy()
    r.setRayStream(0)
    r.render()
    assert r.last_kernel_name not in (STREAM, STREAM12), what
    b = r.readPixels().copy()
    want = oracle.render(vol, p)[0]
    own = [py for py in (range(want.shape[0]) if rows is None else rows) if py >= 0]
    assert_same(a[own], want[own], what + ": replayed frame against the oracle")
    assert_same(a, b, what + ": replayed frame against the gather kernels' frame")
    return a


def n_local(oracle, vol, size, cam, rows=None, spacing=(1.0, 1.0, 1.0)):
    n = S.geometric_counts(oracle, vol, size, cam, spacing=spacing, window=(0, 255))
    return S.local_counts(n, S.local_rows(size[1]) if rows is None else rows)


# ---------------------------------------------------------------------------------------------------------------
# P1: where a ray ends inside a group of eight
# ---------------------------------------------------------------------------------------------------------------
def test_rays_end_at_every_position_of_a_group_by_their_length(vra, oracle):
    """the 12-bit noise ball from the default camera and the edge pose at alpha 1.0, 0.3 and 0.004, in every mode"""
    vol = S.residue_volume(oracle, "u16")
    win = (0, 4095)
    with fresh(vra, C.SIZE, vol) as r:
        r.setWindow(*win)
        for pose in S.RESIDUE_POSES:
            cam = pose_camera(r, pose)
            for mode in S.MODES:
                lut = set_mode(r, mode)
                for alpha in S.RESIDUE_ALPHAS:
                    r.setAlpha(alpha)
                    a = check(r, oracle, vol, S.params(oracle, C.SIZE, cam, alpha, win, mode, lut), f"pose {pose} {mode} alpha {alpha}")
                    assert np.count_nonzero(a[..., 3]) >= 1000
        assert r.rayStreamBuilds() >= len(S.RESIDUE_POSES)


@pytest.mark.parametrize("value,alpha,count", C.END_CASES, ids=[f"ends_after_{c}" for _, _, c in C.END_CASES])
def test_constant_volume_ends_every_ray_at_one_sample(vra, oracle, value, alpha, count):
    """every long ray stops after 8 + r samples, r = 0 .. 7: each position of the second group, in both of its halves"""
    vol = C.constant_volume(value)
    with fresh(vra, C.SIZE, vol) as r:
        r.setWindow(0, 255); r.setAlpha(alpha)
        cam = pose_camera(r, ())
        for mode in ("grey", "grey_tf", "tf"):
            lut = set_mode(r, mode)
            check(r, oracle, vol, S.params(oracle, C.SIZE, cam, alpha, (0, 255), mode, lut), f"constant {value} alpha {alpha} {mode}")
        set_mode(r, "grey")
        _, spp = r.countSamples(per_pixel=True)
        assert np.count_nonzero(spp == count) >= 1000 and spp.max() == count


# ---------------------------------------------------------------------------------------------------------------
# P2 - P4: the bits, the base, the modes
# ---------------------------------------------------------------------------------------------------------------
def test_alternating_bit_patterns(vra, oracle):
    vol = C.pattern_volume()
    with fresh(vra, C.SIZE, vol) as r:
        for pose in S.RESIDUE_POSES:
            cam = pose_camera(r, pose)
            for mode in S.MODES:
                lut = set_mode(r, mode)
                for win, alpha in (((0, 4095), 0.02), ((0x555, 0xAAA), 1.0)):
                    r.setWindow(*win); r.setAlpha(alpha)
                    a = check(r, oracle, vol, S.params(oracle, C.SIZE, cam, alpha, win, mode, lut), f"pattern pose {pose} {mode} window {win}")
                    assert np.count_nonzero(a[..., 3]) >= 1000


@pytest.mark.parametrize("window", C.OFFSET_WINDOWS, ids=lambda w: f"{w[0]}_{w[1]}")
def test_volume_offset_by_1000(vra, oracle, window):
    """[1000, 5095]: the base folds into the window's constants and the tables' bias"""
    vol = C.offset_volume(oracle)
    with fresh(vra, C.SIZE, vol) as r:
        r.setWindow(*window)
        cam = pose_camera(r, S.RESIDUE_POSES[1])
        lit = 0
        for mode in S.MODES:
            lut = set_mode(r, mode)
            for alpha in (0.02, 1.0):
                r.setAlpha(alpha)
                a = check(r, oracle, vol, S.params(oracle, C.SIZE, cam, alpha, window, mode, lut), f"offset window {window} {mode} alpha {alpha}")
                lit += int(np.count_nonzero(a[..., 3]) >= 1000)
        assert lit >= 8                                                # of 10 frames
        assert r.rayStreamBuilds() == 1                                # window, alpha, transfer function and MIP render from one stream


def test_window_too_wide_for_the_shifted_constants(vra, oracle):
    """a window limit of 2^24: the arithmetic path adds the base back as an integer before the convert"""
    vol = C.offset_volume(oracle)
    window = (0, 1 << 24)
    with fresh(vra, C.SIZE, vol) as r:
        r.setWindow(*window); r.setAlpha(1.0)
        cam = pose_camera(r, ())
        for mode in ("grey", "mip"):
            set_mode(r, mode)
            r.setRayStream(2)
            r.render()
            if r.last_kernel_name != STREAM12:
                pytest.fail(f"a window of {window} is not a frame the stream replays: the case needs another window ({r.last_kernel_name})")
            check(r, oracle, vol, S.params(oracle, C.SIZE, cam, 1.0, window, mode), f"wide window {mode}")


# ---------------------------------------------------------------------------------------------------------------
# P5: what cannot be packed keeps the old format
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["span_4096", "u8"])
def test_what_cannot_be_packed_keeps_the_old_format(vra, oracle, kind):
    vol = C.span_4096_volume(oracle) if kind == "span_4096" else S.residue_volume(oracle, "u8")
    win = (0, 4096) if kind == "span_4096" else (0, 255)
    with fresh(vra, C.SIZE, vol) as r:
        r.setWindow(*win); r.setAlpha(0.05)
        cam = pose_camera(r, S.RESIDUE_POSES[1])
        for mode in ("grey", "mip", "tf"):
            lut = set_mode(r, mode)
            check(r, oracle, vol, S.params(oracle, C.SIZE, cam, 0.05, win, mode, lut), f"{kind} {mode}", kernel=STREAM)
        r.setRayStream(2)
        r.render()
        assert r.last_kernel_name == STREAM
        assert r.rayStreamBytes() == S.stream_bytes(n_local(oracle, vol, C.SIZE, cam), vol.dtype.itemsize)


def test_modes_0_and_1_keep_the_old_format_on_a_small_stream(vra, oracle):
    vol = S.residue_volume(oracle, "u16")
    for pack in (0, 1):
        with fresh(vra, C.SIZE, vol, pack=pack) as r:
            r.setWindow(0, 4095); r.setAlpha(0.05)
            cam = pose_camera(r, ())
            check(r, oracle, vol, S.params(oracle, C.SIZE, cam, 0.05, (0, 4095)), f"pack mode {pack}", kernel=STREAM)
            r.setRayStream(2)
            r.render()
            assert r.rayStreamBytes() == S.stream_bytes(n_local(oracle, vol, C.SIZE, cam), 2)
    with pytest.raises(Exception):
        with fresh(vra, C.SIZE, vol, pack=1) as r:
            r.setRayStreamPack(3)


# ---------------------------------------------------------------------------------------------------------------
# P6: the size; cut blocks
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pose", S.PARTIAL_POSES, ids=["default", "edge", "close"])
@pytest.mark.parametrize("size,row_range", S.BYTES_CASES, ids=lambda v: "x".join(map(str, v)) if v else "all")
def test_packed_stream_size_to_the_byte(vra, oracle, size, row_range, pose):
    """a fresh handle, one forced build: sum over blocks of ceil(max n / 8) * 768 bytes + 16, 128 bytes of counts per block and
    blocks + 1 offsets of 8, n from the oracle at alpha_scale = 0"""
    vol = S.residue_volume(oracle, "u16")
    with fresh(vra, size, vol) as r:
        r.setWindow(0, 4095); r.setAlpha(0.05)
        cam = pose_camera(r, pose)
        if row_range is not None:
            r.setRowRange(*row_range)
        r.setRayStream(2)
        r.render()
        assert r.last_kernel_name == STREAM12 and r.rayStreamBuilds() == 1
        rows = S.local_rows(size[1], row_range=row_range)
        n = n_local(oracle, vol, size, cam, rows=rows)
        assert r.rayStreamBytes() == C.packed_stream_bytes(n), (size, row_range, pose)
        assert r.rayStreamBytes() < S.stream_bytes(n, 2) and r.rayStreamBytes() > 16 + S.stream_grid(size[0], len(rows)).blocks * 136 + 8


def test_row_range_and_stripes_inside_blocks(vra, oracle):
    """101x77: rows 13..58 and rank 1 of 3 in cyclic stripes of 16 rows, from the close pose (every lane inside the image has samples)"""
    size = (101, 77)
    vol = S.residue_volume(oracle, "u16")
    win = (500, 3000)
    with fresh(vra, size, vol) as r:
        r.setWindow(*win)
        for mode in ("grey", "mip", "tf"):
            lut = set_mode(r, mode)
            for pose in (S.RESIDUE_POSES[1], S.CLOSE_POSE):
                cam = pose_camera(r, pose)
                for alpha in (0.004, 1.0):
                    r.setAlpha(alpha)
                    what = f"{mode} pose {pose} alpha {alpha}"
                    check(r, oracle, vol, S.params(oracle, size, cam, alpha, win, mode, lut), what + " whole image")
                    r.setRowRange(*S.PARTIAL_ROW_RANGE)
                    rows = S.local_rows(size[1], row_range=S.PARTIAL_ROW_RANGE)
                    p = S.params(oracle, size, cam, alpha, win, mode, lut, row_range=S.PARTIAL_ROW_RANGE)
                    a = check(r, oracle, vol, p, what + " row range", rows=rows)
                    assert np.count_nonzero(a[rows[0]:rows[-1] + 1, :, 3]) > 0
                    r.setRowRange(0, -1)
                    r.setRowStripes(*S.PARTIAL_STRIPES)
                    rows = S.local_rows(size[1], stripes=S.PARTIAL_STRIPES)
                    assert r.localRows() == len(rows)
                    check(r, oracle, vol, S.params(oracle, size, cam, alpha, win, mode, lut), what + " stripes", rows=rows)
                    r.setRowStripes(1, 0, 1)


# ---------------------------------------------------------------------------------------------------------------
# P7: 64-bit offsets; the scan
# ---------------------------------------------------------------------------------------------------------------
def test_packed_record_kernel_with_64_bit_offsets(vra, oracle):
    """the bricked volume just beyond the 24-bit stride limit (tests/offset_limits.py), from the corner camera (its frame reads
    the last voxel) as grey composite and MIP"""
    t = O.THRESHOLDS["bstride_z"]
    dims = t.outside
    assert not O.takes_32bit_path(dims, 2, t.layout)
    vol = O.rand_voxels(np.random.default_rng(sum(dims) + 2), dims, np.uint16)
    assert int(vol.max()) - int(vol.min()) <= C.SPAN12
    size, alpha, win = (96, 64), 0.001, (1500, 2500)
    block = O.corner_camera(E, dims, t.spacing, "front")
    with fresh(vra, size, vol, t.spacing, layout=t.layout) as r:
        r.setWindow(*win); r.setAlpha(alpha)
        r.setCameraBlock(block)
        for mode in ("grey", "mip"):
            set_mode(r, mode)
            p = S.params(oracle, size, block, alpha, win, mode, spacing=t.spacing, threads=8)
            a = check(r, oracle, vol, p, f"64-bit offsets {dims} {mode}")
            assert np.count_nonzero(a[..., 3]) > 0


def test_scan_with_several_blocks_per_thread(vra, oracle):
    """328 x 264: 1496 stream blocks, two per scan thread and idle threads; the offsets past the first 1024 show in the frame and
    in the total"""
    size = (328, 264)
    assert S.SCAN_SIZES[size][1] == 2
    vol = S.residue_volume(oracle, "u16")
    with fresh(vra, size, vol) as r:
        r.setWindow(0, 4095); r.setAlpha(S.SCAN_ALPHA)
        for pose in S.RESIDUE_POSES:
            cam = pose_camera(r, pose)
            a = check(r, oracle, vol, S.params(oracle, size, cam, S.SCAN_ALPHA, (0, 4095)), f"{size} pose {pose}")
            assert np.count_nonzero(a[..., 3]) >= 1000
            r.setRayStream(2)
            r.render()
            if pose == ():
                assert r.rayStreamBytes() == C.packed_stream_bytes(n_local(oracle, vol, size, cam))


# ---------------------------------------------------------------------------------------------------------------
# P8: the mode on a live handle; the copy budget
# ---------------------------------------------------------------------------------------------------------------
def test_switching_the_pack_mode_rebuilds_the_stream(vra, oracle):
    vol = C.offset_volume(oracle)
    win, alpha = (900, 5200), 0.05
    with fresh(vra, C.SIZE, vol) as r:
        r.setWindow(*win); r.setAlpha(alpha)
        cam = pose_camera(r, S.RESIDUE_POSES[1])
        want = oracle.render(vol, S.params(oracle, C.SIZE, cam, alpha, win))[0]
        n = n_local(oracle, vol, C.SIZE, cam)
        r.setRayStream(2)
        for k, (pack, kernel, model) in enumerate([(2, STREAM12, C.packed_stream_bytes(n)), (0, STREAM, S.stream_bytes(n, 2)),
                                                   (2, STREAM12, C.packed_stream_bytes(n))]):
            r.setRayStreamPack(pack)
            for _ in range(2):                                         # the second frame replays what the first built
                r.render()
                assert r.last_kernel_name == kernel, (pack, r.last_kernel_name)
                assert_same(r.readPixels(), want, f"pack mode {pack}, step {k}")
            assert r.rayStreamBuilds() == k + 1
            # (the sample buffer is kept where it is large enough: after the unpacked build it is the unpacked one's)
            assert r.rayStreamBytes() == (model if k < 2 else S.stream_bytes(n, 2))
        r.setRayStreamPack(2)                                          # the same mode again: nothing is rebuilt
        r.render()
        assert r.rayStreamBuilds() == 3


def test_copy_budget_at_the_packed_size(vra, oracle):
    """a budget one byte short of the packed stream refuses it; the packed size itself -- a quarter less than the unpacked
    stream would need -- accepts it"""
    vol = S.residue_volume(oracle, "u16")
    win, alpha = (0, 4095), 0.02
    with fresh(vra, C.SIZE, vol) as r:
        r.setWindow(*win); r.setAlpha(alpha)
        cam = pose_camera(r, ())
        want = oracle.render(vol, S.params(oracle, C.SIZE, cam, alpha, win))[0]
        n = n_local(oracle, vol, C.SIZE, cam)
        packed, unpacked = C.packed_stream_bytes(n), S.stream_bytes(n, 2)
        assert packed < unpacked
        r.setRayStream(0)
        r.render()
        copies = r.residentBytes()[1]
        r.setCopyBudget(copies + packed - 1)
        r.setRayStream(2)
        for _ in range(2):
            r.render()
            assert r.last_kernel_name not in (STREAM, STREAM12)
            assert_same(r.readPixels(), want, "refused")
        assert r.rayStreamBytes() == 0 and r.rayStreamBuilds() == 0 and r.residentBytes()[1] == copies
        r.setCopyBudget(copies + packed)                               # (a new budget re-arms what the old one refused)
        r.render()
        assert r.last_kernel_name == STREAM12
        assert_same(r.readPixels(), want, "accepted")
        assert r.rayStreamBytes() == packed and r.rayStreamBuilds() == 1
        assert r.residentBytes()[1] == copies + packed
