"""The ray-ordered sample stream of a still view (vr_set_ray_stream; volume-renderer_amd/csrc/vr_stream.hip): a frame replayed from
the stream is the gather kernels' frame BIT FOR BIT.  In every case the stream is forced with mode 2 and the frame is compared
(view(np.uint32)) with the same handle's frame at mode 0; the kernel names are asserted so that nothing passes without having
replayed.  What keeps the stream (window, alpha, transfer function, MIP), what must drop it (camera, image, rows, view switch,
voxels), the default rule (64 still launches) and the copy budget / resident-byte accounting follow."""
import numpy as np
import pytest

import u16_volumes

pytestmark = pytest.mark.gpu

STREAM = "raymarch_stream_kernel"
SIZE = (96, 80)          # no multiple of the 32x16 workgroup tiles: the right-hand tiles are partial; some rays miss the box
POSES = (None, (0.0, 0.66, -1.65))
TF_ISO = [0, 60, 140, 255]
TF_COLOUR = [[0.0, 0.0, 0.0, 0.0], [1.0, 0.2, 0.1, 0.1], [0.2, 1.0, 0.3, 0.6], [1.0, 1.0, 1.0, 1.0]]
TF_GREY = [[0.0, 0.0, 0.0, 0.0], [0.3, 0.3, 0.3, 0.1], [0.7, 0.7, 0.7, 0.6], [1.0, 1.0, 1.0, 1.0]]
MODES = ("grey", "mip", "tf", "mip_tf", "grey_tf")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def volume_of(oracle, kind, dims):
    if kind == "u8":
        return oracle.gen_noise_ball(dims, 1, 0x1234)
    if kind == "u16_12bit":
        return oracle.gen_noise_ball(dims, 2, 0x5678)              # <= 4095: the packed copy is resident beside the stream
    return u16_volumes.make(oracle, "white", dims, 77).vol          # 0 .. 65535


def windows_of(kind, mode):
    """windows under which the frame runs the specialised NEAREST kernels (a transfer function's must fit its LDS table); the
    first holds the data's whole range (no clamp), the others clamp on both sides"""
    if kind == "u8":
        return [(0, 255), (20, 200)]
    if kind == "u16_12bit":
        return [(0, 4095), (500, 3000)]
    return [(20000, 40000)] if "tf" in mode else [(0, 65535), (1000, 60000), (30000, 33000)]


def set_mode(r, mode):
    r.setMIP(mode in ("mip", "mip_tf"))
    if mode in ("tf", "mip_tf"):
        r.setTransferFunction(TF_ISO, TF_COLOUR)
    elif mode == "grey_tf":
        r.setTransferFunction(TF_ISO, TF_GREY)
    else:
        r.setTransferFunction()


def set_pose(r, view, pose):
    r.setInitialCameraRotation(rotate_to_top=view == "top", rotate_to_bottom=view == "bottom")
    r.resetCamera()
    if pose is not None:
        r.cameraOrient(*pose)


def replayed_and_gathered(r, what=""):
    """the frame at mode 2 and the same handle's frame at mode 0; asserts which kernels ran"""
    r.setRayStream(2)
    r.render()
    assert r.last_kernel_name == STREAM, (what, r.last_kernel_name)
    a = r.readPixels().copy()
    r.setRayStream(0)
    r.render()
    assert r.last_kernel_name != STREAM, what
    return a, r.readPixels().copy()


def assert_same(a, b, what):
    if not np.array_equal(bits(a), bits(b)):
        bad = np.argwhere(bits(a) != bits(b))
        raise AssertionError(f"{what}: {len(bad)} words differ, first at {bad[0].tolist()}: {a[tuple(bad[0])]!r} vs {b[tuple(bad[0])]!r}")


def fresh(vra, vol=None, size=SIZE, layout=None):
    R = vra.renderer
    r = vra.RendererCore(0)
    r.setup(size)
    assert r.loadShader("VolumeRenderer.cs")
    r.setQuirks(0)
    r.setLayout(R.LAYOUT_BRICKED if layout is None else layout)
    if vol is not None:
        r.setVolume(vol)
    return r


@pytest.mark.parametrize("layout", ["linear", "bricked"])
@pytest.mark.parametrize("kind", ["u8", "u16_12bit", "u16_full"])
@pytest.mark.parametrize("dims", [(64, 64, 64), (40, 52, 36)], ids=["64", "40x52x36"])
def test_parity_matrix(vra, oracle, dims, kind, layout):
    """every mode x view x pose x alpha x window of one (volume, type, layout): 64^3 marches in voxel units, 40x52x36 through the
    certified division; alpha 0.004 ends no ray early, alpha 1.0 ends most within a few samples (the per-wavefront exit, and
    rays that stop inside a group of four)"""
    R = vra.renderer
    vol = volume_of(oracle, kind, dims)
    lit = 0
    with fresh(vra, vol, layout=R.LAYOUT_LINEAR if layout == "linear" else R.LAYOUT_BRICKED) as r:
        for mode in MODES:
            set_mode(r, mode)
            for view in ("front", "top", "bottom"):
                for pose in POSES:
                    set_pose(r, view, pose)
                    for alpha in (0.004, 1.0):
                        r.setAlpha(alpha)
                        for win in windows_of(kind, mode):
                            r.setWindow(*win)
                            what = f"{dims} {kind} {layout} {mode} {view} pose {pose} alpha {alpha} window {win}"
                            a, b = replayed_and_gathered(r, what)
                            assert_same(a, b, what)
                            lit += int(np.count_nonzero(a[..., 3]) > 0)
        assert r.rayStreamBuilds() >= len(MODES) * 3 * len(POSES)     # one build per new geometry at least
    assert lit >= 100                                                  # the frames are not empty


def test_what_keeps_the_stream(vra, oracle):
    """window, alpha, transfer function and MIP render from the SAME stream: no build, the right frame"""
    vol = volume_of(oracle, "u16_12bit", (64, 64, 64))
    with fresh(vra, vol) as r:
        r.setWindow(0, 4095); r.setAlpha(0.02)
        a, b = replayed_and_gathered(r, "first")
        assert_same(a, b, "first")
        builds = r.rayStreamBuilds()
        assert builds == 1 and r.rayStreamBytes() > 0
        changes = [("window", lambda: r.setWindow(300, 2500)), ("alpha", lambda: r.setAlpha(0.7)),
                   ("transfer function", lambda: r.setTransferFunction(TF_ISO, TF_COLOUR)),
                   ("grey transfer function", lambda: r.setTransferFunction(TF_ISO, TF_GREY)),
                   ("no transfer function", lambda: r.setTransferFunction()),
                   ("window again", lambda: r.setWindow(0, 4095)), ("alpha again", lambda: r.setAlpha(0.004))]
        for name, change in changes:
            change()
            a, b = replayed_and_gathered(r, name)
            assert_same(a, b, name)
            assert r.rayStreamBuilds() == builds, name
        # MIP sums its step's divisor in another order (VolumeRenderer.cs:146 against :109): the same bits for this cube, so the
        # same stream; where the step differs the key does (tests/test_ray_geometry_key_cpu.py).  No build while it stays on.
        r.setMIP(True)
        a, b = replayed_and_gathered(r, "mip")
        assert_same(a, b, "mip")
        assert r.rayStreamBuilds() == builds
        r.setWindow(100, 3000); r.setAlpha(0.5)
        a, b = replayed_and_gathered(r, "mip, window and alpha")
        assert_same(a, b, "mip, window and alpha")
        assert r.rayStreamBuilds() == builds


def test_what_must_drop_the_stream(vra):
    """after each change of the ray geometry or of the voxels the frame is the gather kernels' and the stream was built again
    (or is not in use); TRILINEAR and skipping render through the existing kernels"""
    R = vra.renderer
    dims = (64, 64, 64)
    with fresh(vra) as r:
        r.generateSynthetic(R.SYNTH_NOISE_BALL, dims, 2, 0x9E3779B9)
        r.setWindow(0, 4095); r.setAlpha(0.02)
        a, b = replayed_and_gathered(r, "first")
        assert_same(a, b, "first")
        first = a

        def after(name, change, new_frame=True):
            nonlocal first
            builds = r.rayStreamBuilds()
            change()
            r.setRayStream(2)
            r.render()
            replayed = r.last_kernel_name == STREAM
            got = r.readPixels().copy()
            r.setRayStream(0)
            r.render()
            assert r.last_kernel_name != STREAM, name
            want = r.readPixels().copy()
            assert_same(got, want, name)
            assert (replayed and r.rayStreamBuilds() == builds + 1) or not replayed, (name, replayed, builds, r.rayStreamBuilds())
            if new_frame and got.shape == first.shape:
                assert not np.array_equal(bits(got), bits(first)), name + ": the change is visible"
            first = got
            return replayed

        assert after("cameraOrient", lambda: r.cameraOrient(0.0, 0.3, 0.2))
        assert after("zoom", lambda: r.cameraOrient(-1.0, 0.0, 0.0))     # (a dolly of one unit)
        assert after("setup to another size", lambda: r.setup((128, 72)))
        assert after("setRowRange", lambda: r.setRowRange(16, 56), new_frame=False)
        r.setRowRange(0, -1)
        assert after("setRowStripes", lambda: r.setRowStripes(16, 1, 3), new_frame=False)
        r.setRowStripes(1, 0, 1)
        assert after("whole frame again", lambda: None, new_frame=False)
        assert after("setInitialCameraRotation", lambda: r.setInitialCameraRotation(rotate_to_top=True))
        assert after("same dimensions, another seed", lambda: r.generateSynthetic(R.SYNTH_NOISE_BALL, dims, 2, 0x1234567))
        assert after("new voxels and a new window", lambda: (r.generateSynthetic(R.SYNTH_NOISE_BALL, dims, 2, 0x7654321), r.setWindow(200, 3000)))
        assert after("smoothVolume", lambda: r.smoothVolume(sigma_voxels=(1.0, 1.0, 1.0)))
        assert after("another smoothing and a new window", lambda: (r.smoothVolume(sigma_voxels=(2.0, 2.0, 2.0)), r.setWindow(0, 4095)))
        assert after("setLayout", lambda: r.setLayout(R.LAYOUT_LINEAR), new_frame=False)
        assert not after("TRILINEAR", lambda: r.setFilter(R.FILTER_TRILINEAR))
        r.setFilter(R.FILTER_NEAREST)
        r.setWindow(1000, 4095)                                        # a window under which skipping has something to skip
        assert not after("skipping on", lambda: r.setSkipEmpty(True), new_frame=False)
        r.setSkipEmpty(False)
        assert after("skipping off again", lambda: None, new_frame=False)


def test_shard_with_a_compact_grey_alpha_target(vra, oracle):
    """rank 1 of 3 in cyclic stripes of 16 rows into an external compact (grey, alpha) target: the same bits as the gather path"""
    import torch

    R = vra.renderer
    vol = volume_of(oracle, "u16_12bit", (40, 52, 36))
    w, h = SIZE
    with fresh(vra, vol) as r:
        r.setWindow(0, 4095); r.setAlpha(0.05)
        r.setRowStripes(16, 1, 3)
        rows = r.localRows()
        frames = {}
        for mode in (2, 0):
            tgt = torch.full((rows, w, 2), -1.0, dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()
            r.setFramebufferExternal(tgt.data_ptr()); r.setFramebufferCompact(True); r.setFramebufferFormat(R.FB_GREYALPHA32F)
            r.setRayStream(mode)
            r.render()
            r.synchronize()
            assert (r.last_kernel_name == STREAM) == (mode == 2)
            frames[mode] = tgt.cpu().numpy().copy()
            r.setFramebufferExternal(0)
            del tgt
        assert_same(frames[2], frames[0], "shard")
        assert np.count_nonzero(frames[2][..., 1] > 0) > 0


def test_the_default_rule(vra, oracle):
    """mode 1: nothing before the 64th consecutive launch of one geometry; with the measured choice off the 64th replays; a
    camera nudged every frame never builds"""
    vol = volume_of(oracle, "u16_12bit", (64, 64, 64))
    with fresh(vra, vol, size=(256, 256)) as r:
        r.setWindow(0, 4095); r.setAlpha(0.02)
        r.setAutotune(False)                                           # no launch is a measurement: the rule is exact
        r.render()
        old = r.last_kernel_name
        assert r.rayStreamBytes() == 0 and old != STREAM
        for _ in range(62):
            r.render()
            assert r.last_kernel_name == old
        assert r.rayStreamBytes() == 0 and r.rayStreamBuilds() == 0     # 63 still frames
        want = r.readPixels().copy()
        for _ in range(3):
            r.render()                                                 # the 64th, 65th, 66th
            assert r.last_kernel_name == STREAM
            assert_same(r.readPixels(), want, "replayed by the default rule")
        assert r.rayStreamBuilds() == 1 and r.rayStreamBytes() > 0
        for i in range(100):                                           # a moving camera
            r.cameraOrient(0.0, 0.001 if i % 2 else -0.001, 0.0005)
            r.render()
            assert r.last_kernel_name == old
        assert r.rayStreamBuilds() == 1 and r.rayStreamBytes() == 0
    with fresh(vra, vol, size=(256, 256)) as r:                        # the measured choice on (the default): settled long before frame 300
        r.setWindow(0, 4095); r.setAlpha(0.02)
        names = []
        for _ in range(300):
            r.render()
            names.append(r.last_kernel_name)
        assert STREAM not in names[:63]
        assert names[-1] == STREAM and names[-20:] == [STREAM] * 20
        choice = r.last_launch_choice
        r.setRayStream(0)
        r.render()
        assert r.last_launch_choice == choice and r.last_kernel_name != STREAM   # the reported choice is the tuner's either way


def test_budget_and_accounting(vra):
    R = vra.renderer
    dims = (64, 64, 64)
    with fresh(vra) as r:
        r.generateSynthetic(R.SYNTH_NOISE_BALL, dims, 2, 0x9E3779B9)
        r.setWindow(0, 4095); r.setAlpha(0.02)
        r.render()                                                     # the other copies of this configuration are resident now
        want = r.readPixels().copy()
        copies = r.residentBytes()[1]
        r.setCopyBudget(copies + 1024)                                 # below the stream's size
        r.setRayStream(2)
        for _ in range(2):                                             # (a refusal is remembered, not asked again)
            r.render()
            assert r.last_kernel_name != STREAM
            assert_same(r.readPixels(), want, "refused by the budget")
        assert r.rayStreamBytes() == 0 and r.rayStreamBuilds() == 0 and r.residentBytes()[1] == copies
        r.setCopyBudget(r.COPY_BUDGET_AUTO)                            # re-arms it
        r.render()
        assert r.last_kernel_name == STREAM
        assert_same(r.readPixels(), want, "built under the automatic budget")
        stream = r.rayStreamBytes()
        # 2 bytes per sample slot and per pixel of the 8x8 blocks, 8 per block: more than the pixels' counts alone
        assert stream > 2 * 96 * 80 and r.residentBytes()[1] == copies + stream
        r.setCopyBudget(copies + 1024)                                 # lowering the budget frees it again
        assert r.rayStreamBytes() == 0 and r.residentBytes()[1] == copies
        r.setCopyBudget(r.COPY_BUDGET_AUTO)
        r.render()
        assert r.last_kernel_name == STREAM and r.residentBytes()[1] == copies + r.rayStreamBytes()
        r.generateSynthetic(R.SYNTH_NOISE_BALL, dims, 2, 0x51515151)   # the volume is replaced: the stream goes with the voxels
        assert r.rayStreamBytes() == 0 and r.residentBytes()[1] == 0
        r.setRayStream(0)
        r.render()
        assert r.residentBytes()[1] == copies
