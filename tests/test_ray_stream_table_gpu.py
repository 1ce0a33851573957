"""The hybrid classification of the ray stream's replay loop (vr_set_ray_stream_table; csrc/vr_stream.hip: TSHARE): a fixed share
of every lane's samples classified through an LDS table, the rest arithmetically.

Every replayed frame is compared bit for bit with oracle.render, with the same handle's gather-kernel frame and with the same
handle's replay under table mode 0; the kernel name and whether the hybrid was the path taken (rayStreamTableUsed) are asserted
on each.  The cases are tests/ray_stream_table_cases.py's; tests/test_ray_stream_table_cpu.py proves on the CPU that each
reaches what it is named for.

T1  every table mode on the packed and the unpacked stream, an 8-bit twin; the setter's values
T2  windows: the data's range (no clamp, all 4096 entries), one entry more (arithmetic), strictly inside (clamps on both sides),
    the offset volume (the packed base folded into the table's bias), beyond 2^24 (not eligible), MIP, transfer functions
T3  alpha 1 and 0.3 on the residue cameras: rays end by opacity at every position of a group
T4  lanes without samples beside live ones (the edge pose); workgroups none of whose rays has a sample (no table built)
T5  row stripes and a row range on an image cut by its edges
Not covered: streams beyond 2^32 elements or 4 GiB; streams large enough for the automatic mode to take the hybrid.
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


T = _load("ray_stream_table_cases", _HERE / "ray_stream_table_cases.py")
U, C, S = T.U, T.C, T.S
KERNEL = {2: T.STREAM12, 0: T.STREAM}
PACKS = pytest.mark.parametrize("pack", [2, 0], ids=["packed", "unpacked"])


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(bits(got), bits(want)):
        bad = np.argwhere(bits(got) != bits(want))
        raise AssertionError(f"{what}: {len(bad)} words differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}")


def fresh(vra, vol, pack, size=T.SIZE):
    r = vra.RendererCore(0)
    r.setup(size)
    assert r.loadShader("VolumeRenderer.cs")
    r.setQuirks(0)
    r.setLayout(vra.renderer.LAYOUT_BRICKED)
    r.setVolume(vol)
    r.setRayStreamPack(pack)
    return r


def set_mode(r, mode):
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


def replay(r, table, kernel, what):
    r.setRayStreamTable(table)
    r.setRayStream(2)
    r.render()
    assert r.last_kernel_name == kernel, (what, table, r.last_kernel_name)
    return r.readPixels().copy(), r.rayStreamTableUsed()


def check(r, want, what, kernel, hybrid):
    """the frame replayed under table modes 0, 2 and 1 against `want` (the oracle's), the gather kernels' and each other;
    hybrid: whether mode 2 takes the table here.  Mode 1 never does on these streams: they are far below its threshold"""
    assert r.rayStreamBytes() < T.TABLE_MIN_BYTES
    plain, used = replay(r, 0, kernel, what)
    assert not used, what
    assert_same(plain, want, what + ": replay under table mode 0 against the oracle")
    r.setRayStream(0)
    r.render()
    assert r.last_kernel_name not in (T.STREAM, T.STREAM12), what
    gathered = r.readPixels().copy()
    for table, expect in ((2, hybrid), (1, False)):
        a, used = replay(r, table, kernel, what)
        assert used == expect, (what, table, used)
        assert_same(a, want, what + f": table mode {table} against the oracle")
        assert_same(a, gathered, what + f": table mode {table} against the gather kernels' frame")
        assert_same(a, plain, what + f": table mode {table} against table mode 0")
    return plain


# ---------------------------------------------------------------------------------------------------------------
# T1
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,pack", [("u16", 2), ("u16", 0), ("u8", 0)], ids=["u16_packed", "u16_unpacked", "u8"])
def test_every_table_mode(vra, oracle, kind, pack):
    vol = S.residue_volume(oracle, kind)
    win = S.residue_window(kind)
    with fresh(vra, vol, pack) as r:
        assert r.rayStreamTable() == 1                                   # the default
        with pytest.raises(Exception):
            r.setRayStreamTable(3)
        assert r.rayStreamTable() == 1
        r.setWindow(*win); r.setAlpha(0.05)
        cam = pose_camera(r, T.CLOSE_POSE)
        want = oracle.render(vol, S.params(oracle, T.SIZE, cam, 0.05, win))[0]
        a = check(r, want, f"{kind} pack {pack}", KERNEL[pack], True)
        assert np.count_nonzero(a[..., 3]) >= 1000
        assert r.rayStreamBuilds() == 1                                  # a new table mode rebuilds nothing


# ---------------------------------------------------------------------------------------------------------------
# T2
# ---------------------------------------------------------------------------------------------------------------
@PACKS
@pytest.mark.parametrize("name,volume,window,mode,packed_hybrid,unpacked_hybrid", T.CASES, ids=[c[0] for c in T.CASES])
def test_windows_and_modes(vra, oracle, name, volume, window, mode, packed_hybrid, unpacked_hybrid, pack):
    vol = T.volume(oracle, volume)
    hybrid = packed_hybrid if pack == 2 else unpacked_hybrid
    assert hybrid == T.eligible(window, mode, pack == 2, int(vol.min()))
    with fresh(vra, vol, pack) as r:
        r.setWindow(*window)
        cam = pose_camera(r, T.CLOSE_POSE)
        lut = set_mode(r, mode)
        for alpha in T.CASE_ALPHAS:
            r.setAlpha(alpha)
            want = oracle.render(vol, S.params(oracle, T.SIZE, cam, alpha, window, mode, lut))[0]
            a = check(r, want, f"{name} alpha {alpha}", KERNEL[pack], hybrid)
            assert np.count_nonzero(a[..., 3]) >= 1000
        assert r.rayStreamBuilds() == 1


# ---------------------------------------------------------------------------------------------------------------
# T3
# ---------------------------------------------------------------------------------------------------------------
@PACKS
def test_rays_end_by_opacity_at_every_position(vra, oracle, pack):
    vol = S.residue_volume(oracle, "u16")
    win = (0, 4095)
    with fresh(vra, vol, pack) as r:
        r.setWindow(*win)
        for pose in S.RESIDUE_POSES:
            cam = pose_camera(r, pose)
            for mode in ("grey", "mip"):
                set_mode(r, mode)
                for alpha in (1.0, 0.3):
                    r.setAlpha(alpha)
                    want = oracle.render(vol, S.params(oracle, T.SIZE, cam, alpha, win, mode))[0]
                    check(r, want, f"pose {pose} {mode} alpha {alpha}", KERNEL[pack], True)


# ---------------------------------------------------------------------------------------------------------------
# T4
# ---------------------------------------------------------------------------------------------------------------
@PACKS
def test_dead_lanes_and_empty_workgroups(vra, oracle, pack):
    """the edge pose has lanes of n = 0 beside live ones; dollied out, the box covers the middle of the image only, so the outer
    workgroups build no table"""
    vol = T.extremes_volume(oracle)
    win = (1000, 3000)
    with fresh(vra, vol, pack) as r:
        r.setWindow(*win)
        for pose in (T.EDGE_POSE, T.FAR_POSE):
            cam = pose_camera(r, pose)
            for alpha in (0.004, 0.3):
                r.setAlpha(alpha)
                want = oracle.render(vol, S.params(oracle, T.SIZE, cam, alpha, win))[0]
                a = check(r, want, f"pose {pose} alpha {alpha}", KERNEL[pack], True)
                assert np.count_nonzero(a[..., 3]) >= 500 and np.count_nonzero(a[..., 3] == 0) >= 500


# ---------------------------------------------------------------------------------------------------------------
# T5
# ---------------------------------------------------------------------------------------------------------------
@PACKS
def test_row_stripes_and_a_row_range(vra, oracle, pack):
    """an image cut by its edges, a row range that begins and ends inside a block, stripes the image cuts: the launch's own rows
    against the oracle, the whole target against the gather kernels' and against table mode 0"""
    vol = T.extremes_volume(oracle)
    win = (1000, 3000)
    size = S.PARTIAL_SIZES[0]
    with fresh(vra, vol, pack, size) as r:
        r.setWindow(*win); r.setAlpha(0.05)
        cam = pose_camera(r, T.CLOSE_POSE)
        want = oracle.render(vol, S.params(oracle, size, cam, 0.05, win))[0]
        for what in ("row range", "stripes"):
            if what == "row range":
                r.setRowRange(*S.PARTIAL_ROW_RANGE)
                rows = S.local_rows(size[1], row_range=S.PARTIAL_ROW_RANGE)
            else:
                r.setRowRange(0, -1)
                r.setRowStripes(*S.PARTIAL_STRIPES)
                rows = S.local_rows(size[1], stripes=S.PARTIAL_STRIPES)
            assert r.localRows() == len(rows)
            own = [py for py in rows if py >= 0]
            plain, used = replay(r, 0, KERNEL[pack], what)
            assert not used
            a, used = replay(r, 2, KERNEL[pack], what)
            assert used
            r.setRayStream(0)
            r.render()
            assert r.last_kernel_name not in (T.STREAM, T.STREAM12), what
            assert_same(a[own], want[own], what + ": this launch's rows against the oracle")
            assert_same(a, r.readPixels(), what + ": against the gather kernels' frame")
            assert_same(a, plain, what + ": against table mode 0")
            assert np.count_nonzero(a[own][..., 3]) > 0
