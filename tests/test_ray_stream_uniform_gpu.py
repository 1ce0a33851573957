"""The replay loop of the ray-ordered sample stream (csrc/vr_stream.hip) where the lanes of one wavefront part ways: the
shortcut over the per-sample tests, rays that end inside a loaded group, dead lanes, and the addressing of the groups.

Every replayed frame is compared bit for bit with oracle.render first, then with the same handle's gather-kernel frame, and
the kernel name -- `raymarch_stream12_kernel` (pack mode 2) or `raymarch_stream_kernel` (pack mode 0) -- is asserted on each.
The cases are tests/ray_stream_uniform_cases.py's; tests/test_ray_stream_uniform_cpu.py proves on the CPU that each reaches
the branch it is named for.

U1  opacity ends the rays of one wavefront in different units and at every residue (packed, unpacked, an 8-bit twin)
U2  wavefronts whose 64 rays have one length: 16 and 8 (every unit fast), 9 .. 15 (the last unit literal)
U3  lanes without samples beside live ones; exactly one lane much shorter than the other 63
U4  every mode and classification on the close pose, packed and unpacked
U5  addressing: single-group blocks, every block length modulo the held groups, blocks at odd multiples of 768 bytes, the
    stream's size to the byte
Not covered: streams beyond 2^32 elements or 4 GiB.
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


U = _load("ray_stream_uniform_cases", _HERE / "ray_stream_uniform_cases.py")
C, S = U.C, U.S
KERNEL = {2: U.STREAM12, 0: U.STREAM}
FORMAT = {2: "packed", 0: "unpacked"}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(bits(got), bits(want)):
        bad = np.argwhere(bits(got) != bits(want))
        raise AssertionError(f"{what}: {len(bad)} words differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}")


def fresh(vra, vol, pack, spacing=(1.0, 1.0, 1.0)):
    r = vra.RendererCore(0)
    r.setup(U.SIZE)
    assert r.loadShader("VolumeRenderer.cs")
    r.setQuirks(0)
    r.setLayout(vra.renderer.LAYOUT_BRICKED)
    r.setVolume(vol, spacing)
    r.setRayStreamPack(pack)
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


def check(r, oracle, vol, p, what, kernel):
    """the replayed frame against the oracle's, then against the gather kernels' frame of the same handle"""
    r.setRayStream(2)
    r.render()
    assert r.last_kernel_name == kernel, (what, r.last_kernel_name)
    a = r.readPixels().copy()
    r.setRayStream(0)
    r.render()
    assert r.last_kernel_name not in (U.STREAM, U.STREAM12), what
    b = r.readPixels().copy()
    assert_same(a, oracle.render(vol, p)[0], what + ": replayed frame against the oracle")
    assert_same(a, b, what + ": replayed frame against the gather kernels' frame")
    return a


def stream_bytes(n, pack, itemsize):
    rows = S.local_counts(n, S.local_rows(U.SIZE[1]))
    return C.packed_stream_bytes(rows) if pack == 2 else S.stream_bytes(rows, itemsize)


# ---------------------------------------------------------------------------------------------------------------
# U1
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,pack", [("u16", 2), ("u16", 0), ("u8", 0)], ids=["u16_packed", "u16_unpacked", "u8"])
def test_opacity_ends_rays_in_different_units_of_one_wavefront(vra, oracle, kind, pack):
    vol = U.ramp_volume(kind)
    win = U.ramp_window(kind)
    with fresh(vra, vol, pack) as r:
        r.setWindow(*win); r.setAlpha(1.0)
        for pose in (U.CLOSE_POSE, ()):
            cam = pose_camera(r, pose)
            for mode in ("grey", "tf", "grey_tf"):
                lut = set_mode(r, mode)
                a = check(r, oracle, vol, S.params(oracle, U.SIZE, cam, 1.0, win, mode, lut), f"ramp {kind} pose {pose} {mode}", KERNEL[pack])
                assert np.count_nonzero(a[..., 3] >= (S.END_ALPHA if mode == "grey" else 1e-6)) >= 1000


# ---------------------------------------------------------------------------------------------------------------
# U2
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pack", [2, 0], ids=["packed", "unpacked"])
def test_slab_blocks_of_one_ray_length(vra, oracle, pack):
    """one handle, the slab's thickness changed by the spacing: 64 rays of 8 .. 16 samples in the central blocks"""
    vol = S.residue_volume(oracle, "u16")
    win = (0, 4095)
    for length in sorted(U.SLAB_Z):
        spacing = U.slab_spacing(length)
        with fresh(vra, vol, pack, spacing) as r:
            r.setWindow(*win); r.setAlpha(U.SLAB_ALPHA)
            cam = pose_camera(r, U.CLOSE_POSE)
            for mode in ("grey", "mip"):
                set_mode(r, mode)
                p = S.params(oracle, U.SIZE, cam, U.SLAB_ALPHA, win, mode, spacing=spacing)
                a = check(r, oracle, vol, p, f"slab of {length} samples, {mode}", KERNEL[pack])
                assert np.count_nonzero(a[..., 3]) >= 1000
            n = S.geometric_counts(oracle, vol, U.SIZE, cam, spacing=spacing, window=win)
            r.setRayStream(2)
            r.render()
            assert r.rayStreamBytes() == stream_bytes(n, pack, 2), length


# ---------------------------------------------------------------------------------------------------------------
# U3
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pack", [2, 0], ids=["packed", "unpacked"])
def test_mixed_wavefronts(vra, oracle, pack):
    vol = S.residue_volume(oracle, "u16")
    win = (0, 4095)
    with fresh(vra, vol, pack) as r:
        r.setWindow(*win)
        for name in ("edge", "rolled"):
            if name == "edge":
                cam = pose_camera(r, U.EDGE_POSE)
            else:
                cam = U.rolled_camera()
                r.setCameraBlock(cam)
            for mode in ("grey", "mip", "tf"):
                lut = set_mode(r, mode)
                for alpha in (0.004, 0.3, 1.0):
                    r.setAlpha(alpha)
                    a = check(r, oracle, vol, S.params(oracle, U.SIZE, cam, alpha, win, mode, lut), f"{name} {mode} alpha {alpha}", KERNEL[pack])
                    assert np.count_nonzero(a[..., 3]) >= 500


# ---------------------------------------------------------------------------------------------------------------
# U4
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pack", [2, 0], ids=["packed", "unpacked"])
@pytest.mark.parametrize("name,volume,window,mode", U.MODE_CASES, ids=[c[0] for c in U.MODE_CASES])
def test_every_mode_on_the_close_pose(vra, oracle, name, volume, window, mode, pack):
    vol = U.mode_volume(oracle, volume)
    with fresh(vra, vol, pack) as r:
        r.setWindow(*window)
        cam = pose_camera(r, U.CLOSE_POSE)
        lut = set_mode(r, mode)
        for alpha in U.MODE_ALPHAS:
            r.setAlpha(alpha)
            r.setRayStream(2)
            r.render()
            if r.last_kernel_name != KERNEL[pack]:
                pytest.fail(f"{name}: a window of {window} is not a frame the stream replays ({r.last_kernel_name})")
            a = check(r, oracle, vol, S.params(oracle, U.SIZE, cam, alpha, window, mode, lut), f"{name} alpha {alpha}", KERNEL[pack])
            assert np.count_nonzero(a[..., 3]) >= 1000
        assert r.rayStreamBuilds() == 1


# ---------------------------------------------------------------------------------------------------------------
# U5
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pack", [2, 0], ids=["packed", "unpacked"])
def test_addressing_and_the_size_to_the_byte(vra, oracle, pack):
    """the edge pose: single-group blocks, block lengths of every residue modulo the held groups, packed blocks that begin at odd
    multiples of 768 bytes; the stream's size is the model's, as on the parent"""
    vol = S.residue_volume(oracle, "u16")
    win = (0, 4095)
    with fresh(vra, vol, pack) as r:
        r.setWindow(*win)
        cam = pose_camera(r, U.EDGE_POSE)
        n = S.geometric_counts(oracle, vol, U.SIZE, cam, window=win)
        g = U.block_groups(n, FORMAT[pack])
        assert np.count_nonzero(g == 1) >= 1 and np.bincount(g[g > 0] % U.HELD, minlength=U.HELD).min() >= 1
        for alpha in (0.004, 0.05):
            r.setAlpha(alpha)
            check(r, oracle, vol, S.params(oracle, U.SIZE, cam, alpha, win), f"edge pose alpha {alpha}", KERNEL[pack])
        r.setRayStream(2)
        r.render()
        assert r.rayStreamBuilds() == 1
        assert r.rayStreamBytes() == stream_bytes(n, pack, 2)
