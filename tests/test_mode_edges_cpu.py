"""The sampler's edges without a GPU: anchors for the three CPU definitions (tests/iso_ref, tests/shade_ref, tests/reslice_ref)
on thin volumes, at the first and last voxel, with cameras inside / grazing / far and images smaller than a tile -- the cases of
tests/edge_cases.py to which tests/test_mode_edges_gpu.py holds the kernels.  Each anchor ties a definition to something that
does not share its code: oracle.render (pinned to the executed reference), numpy, or a closed form.

The last test shows that the seeded frames the GPU file renders do read the first and the last voxel of the buffer: the share of
frames whose reference bits change with that voxel, per mode and filter (printed with -s, held in its docstring).
"""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

_HERE = Path(__file__).resolve().parent


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


iso_ref = _load("iso_ref_binding", _HERE / "iso_ref" / "binding.py")
reslice_ref = _load("reslice_ref_binding", _HERE / "reslice_ref" / "binding.py")
shade_ref = _load("shade_ref_binding", _HERE / "shade_ref" / "binding.py")
E = _load("edge_cases", _HERE / "edge_cases.py")

QNAN = 0x7FC00000


def test_shared_constants_are_those_of_the_shading_and_isosurface_tests():
    """edge_cases.py keeps no pytest in it, so it restates the coefficients and the transfer function of the existing GPU files"""
    shading = _load("test_shading_gpu_constants", _HERE / "test_shading_gpu.py")
    assert E.COEFS == shading.COEFS and E.TF_ISO == shading.TF_ISO and E.TF_RGBA == shading.TF_RGBA
FILTERS = pytest.mark.parametrize("filt", [0, 1], ids=["nearest", "trilinear"])


@pytest.fixture(scope="session")
def refs(tmp_path_factory):
    d = tmp_path_factory.mktemp("mode_edges_refs")
    return {"iso": (iso_ref, iso_ref.build(d)), "shade": (shade_ref, shade_ref.build(d)), "reslice": (reslice_ref, reslice_ref.build(d))}


def pool_frames(seed, kinds=("random", "corners"), cams=3):
    """every pool entry x both voxel types, `cams` random cameras each; spacing, view, image size and kind are cycled"""
    rng = np.random.default_rng(seed)
    k = 0
    for dims in E.DIMS_POOL:
        for dtype in E.DTYPES:
            vol = E.make_volume(rng, kinds[k % len(kinds)], dims, dtype)
            for _ in range(cams):
                w, h = E.IMAGE_SIZES[k % len(E.IMAGE_SIZES)]
                yield k, dims, dtype, vol, E.SPACINGS[(k // 2) % 2], E.VIEWS[k % 3], (w, h), E.random_camera_block(rng)
                k += 1


def params(oracle, size, cam, spacing, view, filt, **kw):
    return oracle.OracleParams(size[0], size[1], cam=cam, voxel_size=spacing, view_top=int(view == "top"), view_bottom=int(view == "bottom"),
                               filter=filt, **kw)


# ---------------------------------------------------------------------------------------------------------------
# 1: shading at (1, 0, 0) is the composite mode
# ---------------------------------------------------------------------------------------------------------------
@FILTERS
def test_shade_ref_at_unit_ambient_is_the_oracle_on_the_pool(oracle, refs, filt):
    lut = oracle.spline_tf(E.TF_ISO, E.TF_RGBA)
    lit = marched = 0
    for k, dims, dtype, vol, spacing, view, size, cam in pool_frames(11 + filt):
        lo, hi = E.thin_window(dtype)
        p = params(oracle, size, cam, spacing, view, filt, alpha_scale=(0.3, 1.0, 0.02)[k % 3], min_val=lo, max_val=hi,
                   tf_rgba=lut if k % 4 == 1 else None, accum=int(k % 5 == 2))
        want, _, want_spp = oracle.render(vol, p, want_spp=True)
        got = shade_ref.render(refs["shade"][1], vol, p, 1.0, 0.0, 0.0, (16, 1, 128)[k % 3])
        d = E.differ(got, (want, want_spp))
        assert not d, f"frame {k}: {dims} {np.dtype(dtype).name} {spacing} {view} {size}: {d}"
        lit += int((want[..., 3] > 0).sum())
        marched += int((want_spp > 0).sum())
    assert lit > 1000 and marched > 1000, (lit, marched)


# ---------------------------------------------------------------------------------------------------------------
# 2, 3: the isosurface march is the composite march without its dest.a term
# ---------------------------------------------------------------------------------------------------------------
@FILTERS
def test_iso_ref_above_the_maximum_marches_the_oracle_geometry_on_the_pool(oracle, refs, filt):
    """no hit anywhere: depth +inf, RGBA 0, and the per-pixel counts of the oracle at an alpha scale of 0, at which its early
    termination never fires"""
    marched = 0
    for k, dims, dtype, vol, spacing, view, size, cam in pool_frames(21 + filt):
        kw = dict(min_val=0, max_val=E.vmax_of(dtype), accum=int(k % 5 == 2))
        rgba, depth, spp = iso_ref.render(refs["iso"][1], vol, params(oracle, size, cam, spacing, view, filt, **kw), int(vol.max()) + 1, u16_offset=False)
        _, _, want = oracle.render(vol, params(oracle, size, cam, spacing, view, filt, alpha_scale=0.0, **kw), want_spp=True)
        what = f"frame {k}: {dims} {np.dtype(dtype).name} {spacing} {view} {size}"
        assert np.array_equal(spp, want), what
        assert not rgba.any() and np.all(np.isposinf(depth)), what
        marched += int((want > 0).sum())
    assert marched > 1000, marched


@FILTERS
def test_iso_ref_at_or_below_the_minimum_hits_on_the_first_sample_on_the_pool(oracle, refs, filt):
    hits = 0
    for k, dims, dtype, vol, spacing, view, size, cam in pool_frames(31 + filt):
        kw = dict(min_val=0, max_val=E.vmax_of(dtype))
        iso = int(vol.min()) - k % 2                    # at the minimum, or one below it
        rgba, depth, spp = iso_ref.render(refs["iso"][1], vol, params(oracle, size, cam, spacing, view, filt, **kw), iso, u16_offset=False)
        _, _, marched = oracle.render(vol, params(oracle, size, cam, spacing, view, filt, alpha_scale=0.0, **kw), want_spp=True)
        inside = marched > 0
        what = f"frame {k}: {dims} {np.dtype(dtype).name} {spacing} {view} {size} iso {iso}"
        assert np.all(spp[inside] == 1) and np.all(spp[~inside] == 0), what
        assert np.all(np.isfinite(depth[inside])) and np.all(rgba[inside][:, 3] == 1.0), what
        assert np.all(np.isposinf(depth[~inside])) and not rgba[~inside].any(), what
        hits += int(inside.sum())
    assert hits > 1000, hits


# ---------------------------------------------------------------------------------------------------------------
# 4: zero gradients
# ---------------------------------------------------------------------------------------------------------------
def ray_directions(cam, w, h):
    """the shader's ray direction per pixel (VolumeRenderer.cs:61-75), one float32 operation per step: [h, w, 3]"""
    f = np.float32
    c = np.asarray(cam, dtype=np.float32)
    px = (np.arange(w, dtype=np.float32) + f(0.5))[None, :].repeat(h, 0)
    py = (np.arange(h, dtype=np.float32) + f(0.5))[:, None].repeat(w, 1)
    aspect = (f(w) * f(1.0)) / f(h)
    x = aspect * (((f(2.0) * px) / f(w)) - f(1.0))
    y = ((f(2.0) * py) / f(h)) - f(1.0)
    z = np.full_like(x, -c[20])
    zero = np.zeros_like(x)
    rs = f(1.0) / np.sqrt(((zero * zero + z * z) + y * y) + x * x)
    d = [x * rs, y * rs, z * rs, zero * rs]
    m = [((c[r] * d[0] + c[4 + r] * d[1]) + c[8 + r] * d[2]) + c[12 + r] * d[3] for r in range(4)]
    rs = f(1.0) / np.sqrt(((m[3] * m[3] + m[2] * m[2]) + m[1] * m[1]) + m[0] * m[0])
    out = np.stack([m[0] * rs, m[1] * rs, m[2] * rs], axis=-1)
    assert out.dtype == np.float32
    return out


@FILTERS
def test_iso_ref_normal_of_a_zero_gradient_is_minus_the_ray_direction(oracle, refs, filt):
    """`constant` volumes of the whole pool and a 1 x 1 x 1 volume of any value: both central-difference neighbours are the same
    voxel on every axis, G = 0, and the normal is -dir of that pixel's ray, bit for bit; everything is finite where there is a hit"""
    rng = np.random.default_rng(41 + filt)
    hits = 0
    for k, dims in enumerate(E.DIMS_POOL + [(1, 1, 1)] * 3):
        for dtype in E.DTYPES:
            vol = E.make_volume(rng, "constant" if k < len(E.DIMS_POOL) else "random", dims, dtype)
            value = int(vol.flat[0])
            for c in range(3):
                size = E.IMAGE_SIZES[(k + c) % len(E.IMAGE_SIZES)]
                cam = E.random_camera_block(rng)
                p = params(oracle, size, cam, E.SPACINGS[(k + c) % 2], E.VIEWS[(k + c) % 3], filt, min_val=0, max_val=E.vmax_of(dtype))
                rgba, depth, spp, nrm = iso_ref.render(refs["iso"][1], vol, p, value - c % 2, u16_offset=False, want_normal=True)
                hit = np.isfinite(depth)
                what = f"{dims} {np.dtype(dtype).name} value {value} frame {c} {size}"
                assert np.all(spp[hit] == 1) and np.all(spp[~hit] == 0), what
                want = -ray_directions(cam, *size)
                assert np.array_equal(E.bits(nrm[hit]), E.bits(want[hit])), what
                assert np.isfinite(rgba).all() and np.isfinite(nrm).all() and np.all(rgba[hit][:, 3] == 1.0), what
                # the headlight meets the normal head-on: d = |dir|^2, within a few ulp of 1
                assert np.all(rgba[hit][:, :3] > 0.99), what
                hits += int(hit.sum())
    assert hits > 1000, hits


# ---------------------------------------------------------------------------------------------------------------
# 5: reslice against numpy
# ---------------------------------------------------------------------------------------------------------------
def axis_plane(a, centre, step=1.0):
    """the plane through index `centre` of volume axis a (0 = x): columns and rows along the other two axes in x, y, z order, one
    voxel per pixel, pixel (0, 0) on voxel 0"""
    g = np.zeros(12, dtype=np.float32)
    cols, rows = [b for b in range(3) if b != a]
    g[a] = centre
    g[3 + cols] = 1.0
    g[6 + rows] = 1.0
    g[9 + a] = step
    return g, cols, rows


def test_reslice_ref_axis_planes_and_slabs_are_numpy_on_the_pool(refs):
    """planes through voxel centres return the voxels themselves under both filters; slabs of n = 1..9 whole-voxel steps are numpy's
    max, min and sequential float32 mean of the slices inside the volume (an even n is centred between two slices, so that its
    samples fall on voxel centres too); on these volumes most slabs reach outside, where samples do not count"""
    rng = np.random.default_rng(51)
    lib = refs["reslice"][1]
    partial = 0
    for dims in E.DIMS_POOL:
        for dtype in E.DTYPES:
            vol = E.make_volume(rng, "random", dims, dtype)
            lo, hi = E.thin_window(dtype)
            for a in range(3):
                planes = np.moveaxis(vol, 2 - a, 0).astype(np.float32)           # [index along a, rows, cols]
                idx = int(rng.integers(dims[a]))
                for n in range(1, 10):
                    g, cols, rows = axis_plane(a, idx + (0.5 if n % 2 == 0 else 0.0))
                    first = idx - (n - 1) // 2                                     # the slab's samples: first .. first + n - 1
                    inside = [planes[j] for j in range(first, first + n) if 0 <= j < dims[a]]
                    partial += int(len(inside) < n)
                    acc = np.zeros_like(planes[0])
                    for s in inside:
                        acc = (acc + s).astype(np.float32)
                    want = {"mip": np.max(inside, axis=0), "minip": np.min(inside, axis=0), "mean": acc / np.float32(len(inside))}
                    for filt in (0, 1):
                        for red in E.REDUCTIONS:
                            rgba, values, cnt = reslice_ref.render(lib, vol, g, dims[cols], dims[rows], mode=red, n=n, filt=filt, min_val=lo,
                                                                   max_val=hi, u16_offset=False)
                            what = f"{dims} {np.dtype(dtype).name} axis {a} index {idx} n {n} {red} filter {filt}"
                            assert np.all(cnt == len(inside)), what
                            assert np.array_equal(E.bits(values), E.bits(want[red])), what
                            assert np.all(rgba[..., 3] == 1.0), what
    assert partial > 100, partial


@FILTERS
def test_reslice_ref_plane_wholly_outside_is_nan_with_count_zero(refs, filt):
    rng = np.random.default_rng(61 + filt)
    for dims in E.DIMS_POOL:
        vol = E.make_volume(rng, "random", dims, np.uint16)
        for a in range(3):
            for centre in (-0.5 - 1e-3, dims[a] - 0.5, dims[a] + 3.0, -7.0):       # r = centre + 0.5 must lie in [0, dim)
                g, cols, rows = axis_plane(a, centre)
                rgba, values, cnt = reslice_ref.render(refs["reslice"][1], vol, g, dims[cols] + 2, dims[rows] + 2, mode=E.REDUCTIONS[a], n=1, filt=filt,
                                                       min_val=0, max_val=4095)
                assert not cnt.any() and np.all(E.bits(values) == QNAN) and not rgba.any(), (dims, a, centre)


# ---------------------------------------------------------------------------------------------------------------
# 6: the frames of the GPU file read the first and the last voxel
# ---------------------------------------------------------------------------------------------------------------
def sensitivity(refs, oracle, mode, filt):
    """(share of frames that depend on the first voxel, on the last voxel, pool entries without a dependent frame for either)"""
    lut = oracle.spline_tf(E.TF_ISO, E.TF_RGBA)
    dep = {0: [], -1: []}
    per_dims = {0: {}, -1: {}}
    for g in E.thin_cases(mode, filt):
        for case in g.cases:
            for voxel in (0, -1):
                d = E.depends_on_voxel(lambda v: E.thin_reference(refs, oracle, mode, case, filt, lut, v), g.vol, voxel)
                dep[voxel].append(d)
                per_dims[voxel][g.dims] = per_dims[voxel].get(g.dims, 0) + int(d)
    missing = [(voxel, dims) for voxel in (0, -1) for dims, n in per_dims[voxel].items() if n == 0]
    return float(np.mean(dep[0])), float(np.mean(dep[-1])), missing


@pytest.mark.parametrize("mode", ["iso", "shade", "reslice"])
@FILTERS
def test_thin_frames_depend_on_the_first_and_the_last_voxel(oracle, refs, mode, filt):
    """The frames of edge_cases.thin_cases -- the ones test_mode_edges_gpu.py renders -- with the corner voxel at vmax and at 0:
    at least half of them change with the last voxel of the buffer, at least half with the first, and every pool entry has a
    frame that does, for either voxel.  Shares measured (first voxel, last voxel), 208 frames each:
    iso NEAREST 61 % / 64 %, TRILINEAR 64 % / 65 %; shade NEAREST 62 % / 66 %, TRILINEAR 71 % / 75 %; reslice NEAREST 99 % / 100 %,
    TRILINEAR 99 % / 100 % (its planes are laid through both corner voxels: edge_cases.corner_plane).  Six random cameras per volume
    left 128 x 4 x 4 without a frame that reads its first voxel, hence the two aimed ones."""
    first, last, missing = sensitivity(refs, oracle, mode, filt)
    print(f"\n{mode} filter {filt}: {first:.0%} of the frames depend on the first voxel, {last:.0%} on the last")
    assert not missing, missing
    assert first >= 0.5 and last >= 0.5, (first, last)
