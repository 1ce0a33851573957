"""What a launch runs, seen through the public API only: the kernel's name, the candidate bits, the speed copies the launch
gathered from and the handle's device memory, for one frame of each configuration with the measured choice off
(setAutotune(False)), so that the frame runs the rules' first guess (volume-renderer_amd/csrc/launch_plan.cpp,
tile_tables.cpp, RendererCore::prepareLaunch).  The expected values were recorded on an MI355X from the build BEFORE the rules
moved out of RendererCore: they pin the behaviour of that build, not of the code under test.  The rules themselves, on both
sides of every threshold, are tests/test_launch_plan_cpu.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OBLIQUE = (0.0, 0.66, -1.65)         # cameraOrient: no volume axis within 23 degrees of the central ray
# a transfer function whose first entries are transparent (something to skip), grey or coloured
TF_ISO = [0, 400, 4095]
TF_GREY = [[0, 0, 0, 0], [0, 0, 0, 0], [1, 1, 1, 1]]
TF_COLOUR = [[0, 0, 0, 0], [0, 0, 0, 0], [1, 0.5, 0.25, 1]]

# name: (configuration, expected).  Configuration keys (defaults in observe()): n (cube edge), bytes, size, filter, pose, alpha,
# window, skip, stripes (rows, index, count), variant, mode, tf.  Expected: kernel, choice, pack12, tri_copy, resident
# (volume, copies, other)
CASES = {
    "nearest_default_a001": (dict(),
        dict(kernel="raymarch_fast_kernel", choice=2, pack12=3145728, tri_copy=0, resident=[4227584, 3145744, 1230464])),
    "nearest_default_a1": (dict(alpha=1.0),
        dict(kernel="raymarch_fast_kernel", choice=4, pack12=3145728, tri_copy=0, resident=[4227584, 3145744, 1230464])),
    "nearest_oblique_a001": (dict(pose=OBLIQUE),
        dict(kernel="raymarch_relay_kernel", choice=3, pack12=3145728, tri_copy=0, resident=[4227584, 3145744, 1230464])),
    "nearest_oblique_a1": (dict(pose=OBLIQUE, alpha=1.0),
        dict(kernel="raymarch_relay_kernel", choice=5, pack12=3145728, tri_copy=0, resident=[4227584, 3145744, 1230464])),
    "nearest_u8": (dict(bytes=1, window=(0, 255)),
        dict(kernel="raymarch_fast_kernel", choice=2, pack12=0, tri_copy=0, resident=[2113792, 0, 1230464])),
    "nearest_64": (dict(n=64),
        dict(kernel="raymarch_fast_kernel", choice=2, pack12=393216, tri_copy=0, resident=[532992, 393232, 1230464])),
    "nearest_skip": (dict(skip=True, window=(300, 4095)),
        dict(kernel="raymarch_fast_kernel", choice=2, pack12=3145728, tri_copy=0, resident=[4227584, 3145744, 1239856])),
    "nearest_skip_nothing_to_skip": (dict(skip=True),
        dict(kernel="raymarch_fast_kernel", choice=2, pack12=3145728, tri_copy=0, resident=[4227584, 3145744, 1238656])),
    "nearest_stripes_16x2": (dict(stripes=(16, 1, 2)),
        dict(kernel="raymarch_fast_kernel", choice=2, pack12=3145728, tri_copy=0, resident=[4227584, 3145744, 1230144])),
    "nearest_stripes_16x2_oblique_a1": (dict(stripes=(16, 0, 2), pose=OBLIQUE, alpha=1.0),
        dict(kernel="raymarch_relay_kernel", choice=5, pack12=3145728, tri_copy=0, resident=[4227584, 3145744, 1230176])),
    "nearest_variant2": (dict(variant=2, stripes=(16, 1, 2)),
        dict(kernel="raymarch_fast_kernel", choice=0, pack12=3145728, tri_copy=0, resident=[4227584, 3145744, 1230144])),
    "nearest_variant3": (dict(variant=3),
        dict(kernel="raymarch_relay_kernel", choice=1, pack12=3145728, tri_copy=0, resident=[4227584, 3145744, 1230464])),
    "nearest_variant5": (dict(variant=5, alpha=1.0),
        dict(kernel="raymarch_fast_kernel", choice=2, pack12=3145728, tri_copy=0, resident=[4227584, 3145744, 1230464])),
    "nearest_tf_grey": (dict(tf=TF_GREY),
        dict(kernel="raymarch_fast_kernel", choice=2, pack12=3145728, tri_copy=0, resident=[4227584, 3145744, 1234560])),
    "nearest_tf_colour": (dict(tf=TF_COLOUR),
        dict(kernel="raymarch_fast_kernel", choice=2, pack12=3145728, tri_copy=0, resident=[4227584, 3145744, 1234560])),
    "nearest_tf_colour_skip": (dict(tf=TF_COLOUR, skip=True),
        dict(kernel="raymarch_fast_kernel", choice=2, pack12=3145728, tri_copy=0, resident=[4227584, 3145744, 1243952])),
    "nearest_mip": (dict(mip=True),
        dict(kernel="raymarch_fast_kernel", choice=2, pack12=3145728, tri_copy=0, resident=[4227584, 3145744, 1230464])),
    "tri_u8_aligned": (dict(filter=1, bytes=1, window=(0, 255)),
        dict(kernel="raymarch_tslab_kernel", choice=48, pack12=0, tri_copy=2621440, resident=[2113792, 2621456, 1232320])),
    "tri_u8_oblique": (dict(filter=1, bytes=1, window=(0, 255), pose=OBLIQUE),
        dict(kernel="raymarch_tslab_kernel", choice=48, pack12=0, tri_copy=2621440, resident=[2113792, 2621456, 1232320])),
    "tri_u16_aligned": (dict(filter=1),
        dict(kernel="raymarch_tslab_kernel", choice=48, pack12=0, tri_copy=5242880, resident=[4227584, 5242896, 1232320])),
    "tri_u16_oblique": (dict(filter=1, pose=OBLIQUE),
        dict(kernel="raymarch_tslab_kernel", choice=48, pack12=0, tri_copy=15728640, resident=[4227584, 15728688, 1232320])),
    "tri_u16_skip": (dict(filter=1, skip=True, window=(300, 4095)),
        dict(kernel="raymarch_tslab_kernel", choice=48, pack12=0, tri_copy=5242880, resident=[4227584, 5242896, 1242912])),
    "tri_u16_oblique_skip": (dict(filter=1, skip=True, window=(300, 4095), pose=OBLIQUE),
        dict(kernel="raymarch_tslab_kernel", choice=48, pack12=0, tri_copy=15728640, resident=[4227584, 15728688, 1240512])),
    "tri_u16_stripes_16x2_oblique": (dict(filter=1, pose=OBLIQUE, stripes=(16, 1, 2)),
        dict(kernel="raymarch_tslab_kernel", choice=48, pack12=0, tri_copy=15728640, resident=[4227584, 15728688, 1230720])),
    "tri_u16_tf_colour": (dict(filter=1, tf=TF_COLOUR),
        dict(kernel="raymarch_tslab_kernel", choice=48, pack12=0, tri_copy=5242880, resident=[4227584, 5242896, 1236416])),
    "tri_variant6": (dict(filter=1, variant=6),
        dict(kernel="raymarch_tslab_kernel", choice=8, pack12=0, tri_copy=5242880, resident=[4227584, 5242896, 1232320])),
    "tri_variant8": (dict(filter=1, variant=8, pose=OBLIQUE),
        dict(kernel="raymarch_tslab_kernel", choice=24, pack12=0, tri_copy=15728640, resident=[4227584, 15728688, 1232320])),
    "tri_variant9": (dict(filter=1, variant=9, pose=OBLIQUE),
        dict(kernel="raymarch_tslab_kernel", choice=32, pack12=0, tri_copy=15728640, resident=[4227584, 15728688, 1232320])),
    "tri_variant9_stripes_16x2": (dict(filter=1, variant=9, pose=OBLIQUE, stripes=(16, 1, 2)),
        dict(kernel="raymarch_tslab_kernel", choice=32, pack12=0, tri_copy=15728640, resident=[4227584, 15728688, 1231040])),
    "iso": (dict(n=64, mode="iso"),
        dict(kernel="raymarch_iso_kernel", choice=0, pack12=0, tri_copy=0, resident=[532992, 0, 1537056])),
    "iso_skip": (dict(n=64, mode="iso", skip=True),
        dict(kernel="raymarch_iso_kernel", choice=0, pack12=0, tri_copy=0, resident=[532992, 0, 1538080])),
    "reslice": (dict(n=64, mode="reslice"),
        dict(kernel="reslice_kernel", choice=0, pack12=0, tri_copy=0, resident=[532992, 0, 1537056])),
    "shaded": (dict(n=64, mode="shade"),
        dict(kernel="raymarch_shade_kernel", choice=0, pack12=0, tri_copy=0, resident=[532992, 0, 1229856])),
    "shaded_skip_tf": (dict(n=64, mode="shade", skip=True, tf=TF_COLOUR),
        dict(kernel="raymarch_shade_kernel", choice=0, pack12=0, tri_copy=0, resident=[532992, 0, 1234976])),
    "shaded_mip_is_a_ray_march": (dict(n=64, mode="shade", mip=True),
        dict(kernel="raymarch_fast_kernel", choice=2, pack12=393216, tri_copy=0, resident=[532992, 393232, 1230464])),
}


def observe(vra, cfg):
    """one frame of the configuration on a fresh handle: (what the launch reports, the frame)"""
    R = vra.renderer
    c = dict(n=128, bytes=2, size=(320, 240), filter=0, pose=None, alpha=0.01, window=(0, 4095), skip=False, stripes=None, variant=0,
             mode=None, tf=None, mip=False)
    c.update(cfg)
    with vra.RendererCore(0) as r:
        r.setup(c["size"]); assert r.loadShader("VolumeRenderer.cs"); r.setQuirks(0)
        r.setAutotune(False)
        r.generateSynthetic(R.SYNTH_NOISE_BALL, (c["n"],) * 3, c["bytes"], 0x9E3779B9)
        r.setWindow(*c["window"]); r.setAlpha(c["alpha"]); r.setMIP(c["mip"])
        r.setFilter(c["filter"])
        if c["pose"]:
            r.cameraOrient(*c["pose"])
        if c["tf"]:
            r.setTransferFunction(TF_ISO, c["tf"])
        r.setSkipEmpty(c["skip"])
        if c["stripes"]:
            r.setRowStripes(*c["stripes"])
        r.setKernelVariant(c["variant"])
        if c["mode"] == "iso":
            r.setIsosurface(True, 1500)
        elif c["mode"] == "reslice":
            h = c["n"] / 2.0
            r.setReslice(True, (0.0, 0.0, h), (c["n"] / c["size"][0], 0, 0), (0, c["n"] / c["size"][1], 0), (0, 0, 1), mode="mean", n=3)
        elif c["mode"] == "shade":
            r.setShading(True)
        r.render()
        seen = dict(kernel=r.last_kernel_name, choice=r.last_launch_choice, pack12=r.pack12Bytes(), tri_copy=r.trilinearCopyBytes(),
                    resident=list(r.residentBytes()))
        return seen, r.readPixels()


@pytest.mark.parametrize("name", list(CASES))
def test_the_launch_is_the_one_the_rules_set(vra, name):
    cfg, want = CASES[name]
    seen, frame = observe(vra, cfg)
    print(name, seen)
    assert seen == want
    assert np.isfinite(frame).all()
