"""vr_smooth_volume at the limits of its LDS ring, its column segments, its x tiles and its z slabs (tests/smoothing_cases.py;
tests/test_smoothing_cases_cpu.py shows that each case reaches what it is for and that tests/test_smoothing_gpu.py reaches none
of it).  Every comparison is the whole volume read back against tests/smooth_ref/smooth_ref.c, bit for bit, on 8- and 16-bit
voxels and, where not stated otherwise, in both layouts.

  E1  both rings at their last and first radius (r = 8, 9, 24), full, on y and on z, in every input / output instance, over
      columns of four segments with a short last one
  E2  every radius 1 .. 24 along x, y, z alone and together
  E3  two and three x tiles, radii up to 24 across their seams
  E4  z slabs at the largest radius: one, two and 17 output planes per slab, a slab without a halo, a volume thinner than a
      slab, the refusal one plane below
  E5  constant volumes, a checkerboard, zero corners in a saturated volume, single voxels

Not covered: an exact .5 tie before the final rounding.  It cannot be constructed from Gaussian weights, so half-to-even is
exercised only as far as the random volumes reach it.
"""
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


S = _load("smoothing_cases", HERE / "smoothing_cases.py")
smooth_ref = _load("smooth_ref_binding", HERE / "smooth_ref" / "binding.py")

DTYPES = pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])


@pytest.fixture(scope="module")
def smoothlib(tmp_path_factory):
    return smooth_ref.build(tmp_path_factory.mktemp("smooth_ref_edges"))


@pytest.fixture(scope="module")
def handle(vra):
    """one renderer with a 64 x 48 target"""
    r = vra.RendererCore(0)
    r.setup((64, 48))
    assert r.loadShader("VolumeRenderer.cs")
    yield r
    r.close()


def weights_for(vra, sigmas):
    return tuple(vra.smooth_weights(s) if s > 0 else None for s in sigmas)


_REF = {}


def reference(vra, smoothlib, key, vol, sig):
    """the CPU definition's result, computed once per (volume key, sigmas) and shared"""
    k = (key, tuple(float(s) for s in sig))
    if k not in _REF:
        out = smooth_ref.smooth(smoothlib, vol, weights_for(vra, sig))
        out.setflags(write=False)
        _REF[k] = out
    return _REF[k]


def first_difference(got, want):
    bad = np.argwhere(got != want)
    z, y, x = bad[0]
    return f"{len(bad)} voxels differ, first (x {x}, y {y}, z {z}): {got[z, y, x]} vs {want[z, y, x]}"


def layouts(vra):
    return (vra.renderer.LAYOUT_LINEAR, vra.renderer.LAYOUT_BRICKED)


def smooth_and_compare(vra, smoothlib, r, key, vol, sig, what):
    """one call on the loaded volume `vol`, the voxels read back against the reference; returns (got, want)"""
    r.smoothVolume(sigma_voxels=sig)
    assert r.smoothing == tuple(float(np.float32(s)) for s in sig)
    got = r.readVolume()
    want = reference(vra, smoothlib, key, vol, sig)
    assert np.array_equal(got, want), f"{what} sigma {sig}: " + first_difference(got, want)
    return got, want


# ---------------------------------------------------------------------------------------------------------------
# E1: the column rings
# ---------------------------------------------------------------------------------------------------------------
SIGMA_SETS = {"r8": S.SUBSETS(2.5), "r9": S.SUBSETS(3.0), "r24": S.SUBSETS(8.0), "mixed": S.MIXED}


@pytest.mark.parametrize("sigmas", list(SIGMA_SETS))
@DTYPES
@pytest.mark.parametrize("name", list(S.COLUMN_PLANS))
def test_column_rings_full_and_wrapping_over_interior_and_short_segments(vra, smoothlib, handle, name, dtype, sigmas):
    r = handle
    vol = S.random_volume(name, dtype)
    key = (name, np.dtype(dtype).name)
    for layout in layouts(vra):
        r.setLayout(layout)
        r.setVolume(vol)
        for sig in SIGMA_SETS[sigmas]:
            smooth_and_compare(vra, smoothlib, r, key, vol, sig, f"{name} {key[1]} layout {layout}")


# ---------------------------------------------------------------------------------------------------------------
# E2: every radius
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axes", ["x", "y", "z", "xyz"])
@DTYPES
def test_every_radius(vra, smoothlib, handle, dtype, axes):
    r = handle
    vol = S.random_volume("SWEEP", dtype)
    key = ("SWEEP", np.dtype(dtype).name)
    for layout in layouts(vra):
        r.setLayout(layout)
        r.setVolume(vol)
        for radius in range(1, S.MAX_RADIUS + 1):
            s = S.sweep_sigma(radius)
            sig = tuple(s if a in axes else 0.0 for a in "xyz")
            smooth_and_compare(vra, smoothlib, r, key, vol, sig, f"radius {radius} along {axes}, {key[1]} layout {layout}")


# ---------------------------------------------------------------------------------------------------------------
# E3: the x pass across tiles
# ---------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("name", ["XT", "XT_ALIGNED", "XT_EDGE"])
def test_x_pass_across_tiles(vra, smoothlib, handle, name, dtype):
    r = handle
    vol = S.random_volume(name, dtype)
    key = (name, np.dtype(dtype).name)
    for layout in layouts(vra):
        r.setLayout(layout)
        r.setVolume(vol)
        for sx in S.X_SIGMAS:
            for sig in ((sx, 0.0, 0.0), (sx, 1.0, 1.0)):
                what = f"{name} {key[1]} layout {layout}"
                if name == "XT" and S.radius(sx) == S.MAX_RADIUS:
                    # first the voxels whose neighbourhood crosses a tile seam, on their own: a failure names the seam
                    r.smoothVolume(sigma_voxels=sig)
                    got = r.readVolume()
                    want = reference(vra, smoothlib, key, vol, sig)
                    for cols in S.XT_SEAM_COLUMNS:
                        g, w = got[:, :, cols], want[:, :, cols]
                        assert np.array_equal(g, w), (f"{what} sigma {sig}, columns x = {cols.start} .. {cols.stop - 1} around the tile seam: "
                                                      + first_difference(g, w) + f" (x relative to {cols.start})")
                smooth_and_compare(vra, smoothlib, r, key, vol, sig, what)


# ---------------------------------------------------------------------------------------------------------------
# E4: z slabs at the largest radius
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.SLAB_CASES, ids=lambda c: "s" + "_".join(f"{s:g}" for s in c[0]) + f"-{c[1]}planes")
@DTYPES
def test_slabs_at_the_largest_radius(vra, smoothlib, handle, dtype, case):
    sig, planes, _ = case
    r = handle
    vol = S.random_volume("BOTH", dtype)
    r.setLayout(vra.renderer.LAYOUT_BRICKED)
    r.setVolume(vol)
    try:
        r.setSmoothingWorkspace(S.workspace_bytes(S.SHAPES["BOTH"], planes))
        smooth_and_compare(vra, smoothlib, r, ("BOTH", np.dtype(dtype).name), vol, sig, f"BOTH {np.dtype(dtype).name}, {planes} planes")
    finally:
        r.setSmoothingWorkspace(0)


@DTYPES
def test_a_volume_thinner_than_a_slab_runs_in_one_piece_or_not_at_all(vra, smoothlib, handle, dtype):
    r = handle
    R = vra.renderer
    vol = S.random_volume("THIN", dtype)
    key = ("THIN", np.dtype(dtype).name)
    r.setLayout(R.LAYOUT_BRICKED)
    r.setVolume(vol)
    try:
        # a single pass needs no planes: the state the refused call must leave
        before = (0.0, 2.5, 0.0)
        r.setSmoothingWorkspace(S.workspace_bytes(S.SHAPES["THIN"], S.THIN_PLANES_REFUSED))
        kept, _ = smooth_and_compare(vra, smoothlib, r, key, vol, before, "THIN, one pass")
        with pytest.raises(vra.VRError) as e:
            r.smoothVolume(sigma_voxels=S.THIN_SIGMA)
        assert e.value.code == R.VR_E_NOMEM
        assert r.smoothing == before and np.array_equal(r.readVolume(), kept)
        r.setSmoothingWorkspace(S.workspace_bytes(S.SHAPES["THIN"], S.THIN_PLANES_OK))
        kept, _ = smooth_and_compare(vra, smoothlib, r, key, vol, S.THIN_SIGMA, f"THIN, {S.THIN_PLANES_OK} planes")
        r.setSmoothingWorkspace(S.workspace_bytes(S.SHAPES["THIN"], S.THIN_PLANES_REFUSED))
        with pytest.raises(vra.VRError) as e:
            r.smoothVolume(sigma_voxels=S.THIN_SIGMA)
        assert e.value.code == R.VR_E_NOMEM
        assert r.smoothing == S.THIN_SIGMA and np.array_equal(r.readVolume(), kept)
    finally:
        r.setSmoothingWorkspace(0)


# ---------------------------------------------------------------------------------------------------------------
# E5: values
# ---------------------------------------------------------------------------------------------------------------
BIG = (8.0, 8.0, 8.0)


@pytest.mark.parametrize("dtype,value", [(np.uint8, 0), (np.uint8, 255), (np.uint16, 0), (np.uint16, 255), (np.uint16, 65535)],
                         ids=["u8-0", "u8-255", "u16-0", "u16-255", "u16-65535"])
def test_constant_volumes_come_back_unchanged(vra, handle, dtype, value):
    r = handle
    nx, ny, nz = S.SHAPES["BOTH"]
    vol = np.full((nz, ny, nx), value, dtype=dtype)
    for layout in layouts(vra):
        r.setLayout(layout)
        r.setVolume(vol)
        r.smoothVolume(sigma_voxels=BIG)
        got = r.readVolume()
        assert np.array_equal(got, vol), f"constant {value}, layout {layout}: " + first_difference(got, vol)


@pytest.mark.parametrize("kind", S.VALUE_CASES)
@DTYPES
def test_extreme_values_at_the_largest_radius(vra, smoothlib, handle, dtype, kind):
    r = handle
    vol = S.value_volume(kind, dtype)
    for layout in layouts(vra):
        r.setLayout(layout)
        r.setVolume(vol)
        got, _ = smooth_and_compare(vra, smoothlib, r, (kind, np.dtype(dtype).name), vol, BIG, f"{kind} {np.dtype(dtype).name} layout {layout}")
        assert not np.array_equal(got, vol)
