"""16-bit volumes over the whole value range, without a GPU: the CPU definitions (oracle.render, tests/iso_ref, tests/shade_ref,
tests/reslice_ref) satisfy the two exact invariances that tests/test_u16_full_range_gpu.py holds the kernels to.

Scale by 16: a 12-bit volume V with the stored window [lo, hi] and 16 * V with [16 * lo, 16 * hi] give the same bits -- every
fp32 operand is scaled by a power of two -- for both filters, in every mode.  Offset by B: V + B with [lo + B, hi + B] gives the
same bits under NEAREST, because (float)(v + B) - (float)(lo + B) is exact; a reslice `mean` over more than one sample is
excluded by definition (the sum of shifted values rounds differently), and so is TRILINEAR (lerps of larger operands do).
12-bit frames are pinned to the executed-reference goldens, so the invariances carry that to the whole 16-bit range.

All windows and iso values here are in STORED units unless a test says otherwise (VR_QUIRK_U16_OFFSET adds 1000 on the way in).
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
u16 = _load("u16_volumes", _HERE / "u16_volumes.py")

N_VOLUMES = 12
TF_ISO = [0, 60, 140, 255]
TF_RGBA = [[0.2, 0.9, 0.1, 0.0], [0.9, 0.3, 0.2, 0.4], [1.0, 0.8, 0.6, 0.8], [0.5, 0.5, 1.0, 1.0]]
COEFS = [(0.15, 0.65, 0.2, 16), (1.0, 0.0, 0.0, 16), (0.3, 1.7, 0.6, 1), (0.0, 0.9, 0.35, 128), (0.05, 0.4, 0.9, 2)]
POSES = [dict(), dict(zenith=0.5, azimuth=0.8), dict(zenith=-0.7, azimuth=2.2), dict(zoom_in=3), dict(zoom_in=2, zenith=0.3, azimuth=-0.4),
         dict(zenith=1.2, azimuth=0.1)]


@pytest.fixture(scope="session")
def isolib(tmp_path_factory):
    return iso_ref.build(tmp_path_factory.mktemp("iso_ref_u16"))


@pytest.fixture(scope="session")
def rslib(tmp_path_factory):
    return reslice_ref.build(tmp_path_factory.mktemp("reslice_ref_u16"))


@pytest.fixture(scope="session")
def shadelib(tmp_path_factory):
    return shade_ref.build(tmp_path_factory.mktemp("shade_ref_u16"))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    """tuples of float32 frames (compared by bits) and integer counts"""
    return all(np.array_equal(bits(x), bits(y)) if x.dtype == np.float32 else np.array_equal(x, y) for x, y in zip(a, b))


def orbit_cam(oracle, zenith=0.0, azimuth=0.0, zoom_in=0):
    c = oracle.Camera()
    for _ in range(zoom_in):
        c.orient(1.0, 0.0, 0.0)
    if zenith or azimuth:
        c.orient(0.0, zenith, azimuth)
    return c.block()


def seeded_case(oracle, seed):
    """a 12-bit volume of random dims 9..39 with anisotropic spacing, its three full-range relatives, a window, a pose, a frame"""
    rng = np.random.default_rng(1000 + seed)
    dims = tuple(int(v) for v in rng.integers(9, 40, size=3))
    if seed % 3 == 0:
        dims = (dims[0] | 1, dims[1], dims[2])
    spacing = tuple(float(v) for v in rng.uniform(0.5, 2.0, size=3).round(2))
    field = ("ball", "smooth", "rand")[seed % 3]
    twin = u16.twin12(oracle, rng, dims, field)
    rel = [u16.Volume("scaled_" + field, (twin.astype(np.uint32) * 16).astype(np.uint16), twin, 16, 0)]
    rel += [u16.Volume(f"shifted{b}", (twin.astype(np.uint32) + b).astype(np.uint16), twin, 1, b) for b in u16.SHIFTS]
    for v in rel:
        u16.check(v)
    lo, hi = int(rng.integers(0, 1300)), int(rng.integers(2000, 4096))
    cam = orbit_cam(oracle, **POSES[int(rng.integers(len(POSES)))])
    w, h = int(rng.integers(24, 49)), int(rng.integers(17, 41))
    return rng, dims, spacing, twin, rel, (lo, hi), cam, (w, h)


def relatives(rel, filt):
    """scale by 16 holds for both filters, the offsets for NEAREST only"""
    return [v for v in rel if v.shift == 0 or filt == 0]


@pytest.mark.parametrize("filt", [0, 1], ids=["nearest", "trilinear"])
def test_oracle_frames_are_scale_and_offset_invariant(oracle, filt):
    lut = oracle.spline_tf(TF_ISO, TF_RGBA)
    lit = compared = 0
    for seed in range(N_VOLUMES):
        _, dims, spacing, twin, rel, (lo, hi), cam, (w, h) = seeded_case(oracle, seed)
        for mip in (0, 1):
            for tf in (None, lut):
                for accum in (0, 1):
                    for alpha in (0.05, 1.0):
                        kw = dict(cam=cam, alpha_scale=alpha, voxel_size=spacing, is_mip=mip, filter=filt, accum=accum, tf_rgba=tf)
                        base = oracle.render(twin, oracle.OracleParams(w, h, min_val=lo, max_val=hi, **kw), want_spp=True)
                        for v in relatives(rel, filt):
                            flo, fhi = u16.twin_window(v, lo, hi)
                            got = oracle.render(v.vol, oracle.OracleParams(w, h, min_val=flo, max_val=fhi, **kw), want_spp=True)
                            assert same((got[0], got[2]), (base[0], base[2])) and got[1] == base[1], (seed, v.kind, dims, mip, tf is not None, accum, alpha)
                            lit += int((got[0][..., 3] > 0).sum())
                            compared += 1
    assert compared == N_VOLUMES * 16 * (3 if filt == 0 else 1)
    assert lit > 1000, lit


@pytest.mark.parametrize("filt", [0, 1], ids=["nearest", "trilinear"])
def test_isosurface_reference_is_scale_and_offset_invariant(oracle, isolib, filt):
    lut = oracle.spline_tf(TF_ISO, TF_RGBA)
    with_hits = without_hits = lit = 0
    for seed in range(N_VOLUMES):
        rng, dims, spacing, twin, rel, (lo, hi), cam, (w, h) = seeded_case(oracle, seed)
        vmin, vmax = int(twin.min()), int(twin.max())
        quirk = seed % 2 == 1                                     # odd seeds work in HU = stored - 1000, as the C ABI does by default
        for iso in (int(rng.integers(vmin + 1, vmax + 1)), (vmin + vmax) // 2, vmax + 1):
            p = oracle.OracleParams(w, h, cam=cam, voxel_size=spacing, min_val=lo, max_val=hi, filter=filt, tf_rgba=lut if seed % 4 < 2 else None)
            base = iso_ref.render(isolib, twin, p, iso - 1000 if quirk else iso, u16_offset=quirk)
            hit = np.isfinite(base[1])
            with_hits += int(hit.any())
            without_hits += int(not hit.any())
            lit += int(hit.sum())
            for v in relatives(rel, filt):
                p.min_val, p.max_val = u16.twin_window(v, lo, hi)
                stored = v.scale * iso + v.shift
                got = iso_ref.render(isolib, v.vol, p, stored - 1000 if quirk else stored, u16_offset=quirk)
                assert same(got, base), (seed, v.kind, dims, iso, quirk)
    assert with_hits > 0 and without_hits > 0 and lit > 1000, (with_hits, without_hits, lit)


@pytest.mark.parametrize("filt", [0, 1], ids=["nearest", "trilinear"])
def test_shading_reference_is_scale_and_offset_invariant(oracle, shadelib, filt):
    lut = oracle.spline_tf(TF_ISO, TF_RGBA)
    lit = 0
    for seed in range(N_VOLUMES):
        _, dims, spacing, twin, rel, (lo, hi), cam, (w, h) = seeded_case(oracle, seed)
        for tf in (None, lut):
            for alpha in (0.05, 1.0):
                coef = COEFS[(seed + int(alpha == 1.0)) % len(COEFS)]
                kw = dict(cam=cam, alpha_scale=alpha, voxel_size=spacing, filter=filt, accum=seed % 2, tf_rgba=tf)
                base = shade_ref.render(shadelib, twin, oracle.OracleParams(w, h, min_val=lo, max_val=hi, **kw), *coef)
                lit += int((base[0][..., 3] > 0).sum())
                for v in relatives(rel, filt):
                    flo, fhi = u16.twin_window(v, lo, hi)
                    got = shade_ref.render(shadelib, v.vol, oracle.OracleParams(w, h, min_val=flo, max_val=fhi, **kw), *coef)
                    assert same(got, base), (seed, v.kind, dims, tf is not None, alpha, coef)
    assert lit > 1000, lit


@pytest.mark.parametrize("filt", [0, 1], ids=["nearest", "trilinear"])
def test_reslice_reference_is_scale_and_offset_invariant(vra, oracle, rslib, filt):
    lut = oracle.spline_tf(TF_ISO, TF_RGBA)
    with_nan = lit = 0
    for seed in range(N_VOLUMES):
        rng, dims, spacing, twin, rel, (lo, hi), _, (w, h) = seeded_case(oracle, seed)
        centre = (np.array(dims, dtype=np.float64) - 1) / 2 + rng.uniform(-0.15, 0.15, size=3) * np.array(dims)
        pixel = rng.uniform(0.5, 1.6) * min(dims) / max(w, h)
        geom = vra.reslice_geometry(dims, (1, 1, 1), centre, rng.normal(size=3), rng.normal(size=3), pixel, float(rng.uniform(0.2, 1.5)), (w, h))
        for mode in ("mip", "minip", "mean"):
            for n in (1, 7, 64):
                kw = dict(mode=mode, n=n, filt=filt, tf_rgba=lut if seed % 2 else None)
                base = reslice_ref.render(rslib, twin, geom, w, h, min_val=lo, max_val=hi, u16_offset=False, **kw)
                base_hu = reslice_ref.render(rslib, twin, geom, w, h, min_val=lo, max_val=hi, u16_offset=True, **kw)
                nan = np.isnan(base[1])
                with_nan += int(nan.any())
                lit += int((base[2] > 0).sum())
                assert np.array_equal(nan, base[2] == 0)
                for v in relatives(rel, filt):
                    if v.shift and mode == "mean" and n > 1:
                        continue                                  # excluded by definition: the sum of shifted values rounds differently
                    flo, fhi = u16.twin_window(v, lo, hi)
                    got = reslice_ref.render(rslib, v.vol, geom, w, h, min_val=flo, max_val=fhi, u16_offset=False, **kw)
                    what = (seed, v.kind, dims, mode, n)
                    assert same((got[0], got[2]), (base[0], base[2])), what
                    # the read-back values with the +1000 offset off: exactly 16 x, or exactly + B (integers, or one sample)
                    want = base[1] * np.float32(v.scale) + np.float32(v.shift)
                    assert np.array_equal(bits(got[1][~nan]), bits(want[~nan])) and np.isnan(got[1][nan]).all(), what
                    # ... and with it on, the same picture and the values 1000 lower (what a read-back in HU is)
                    hu = reslice_ref.render(rslib, v.vol, geom, w, h, min_val=flo, max_val=fhi, u16_offset=True, **kw)
                    assert same((hu[0], hu[2]), (base_hu[0], base_hu[2])), what
                    assert np.array_equal(bits(hu[1][~nan]), bits(got[1][~nan] - np.float32(1000.0))), what
    assert with_nan > 0 and lit > 1000, (with_nan, lit)


def mean_slab_samples(vol, geom, w, h, n):
    """the NEAREST samples of reslice_ref.c for a slab along z under an axial plane: [n, h, w] values and the inside mask [n]"""
    nz, ny, nx = vol.shape
    g = np.asarray(geom, dtype=np.float32)
    assert np.array_equal(g[3:9], np.array([1, 0, 0, 0, 1, 0], dtype=np.float32)) and g[0] == 0 and g[1] == 0 and g[9] == 0 and g[10] == 0
    assert (w, h) == (nx, ny)
    k = np.arange(n)
    c = (2 * k - (n - 1)).astype(np.float32) * np.float32(0.5)
    r = ((g[2] + (c * g[11]).astype(np.float32)).astype(np.float32) + np.float32(0.5)).astype(np.float32)
    inside = (r >= 0) & (r < np.float32(nz))
    return vol[r[inside].astype(np.int64)].astype(np.float32), inside


def test_the_order_of_a_full_range_mean_is_visible_in_the_bits(oracle, rslib):
    """NEAREST `mean`, n = 1024: at 12 bits the sum stays below 2^24 and is exact in any order; at 16 bits it reaches 3e7 and
    rounds on the way, so the sequential fp32 sum the definition prescribes differs from the exactly rounded one"""
    vol, geom, (w, h) = u16.mean_order_case(oracle)
    _, values, cnt = reslice_ref.render(rslib, vol, geom, w, h, mode="mean", n=1024, filt=0, min_val=0, max_val=65535, u16_offset=False)
    samples, inside = mean_slab_samples(vol, geom, w, h, 1024)
    assert inside.all() and np.all(cnt == 1024)
    acc = np.zeros((h, w), dtype=np.float32)
    for s in samples:
        acc = (acc + s).astype(np.float32)
    assert float(acc.max()) > 2.0 ** 24
    assert np.array_equal(bits(values), bits(acc / np.float32(1024)))                     # the definition: sequential, slab order
    exact = samples.astype(np.float64).sum(axis=0).astype(np.float32) / np.float32(1024)  # the same samples, summed exactly
    differ = int((bits(values) != bits(exact)).sum())
    assert differ > 0
    # and the 12-bit twin of that geometry hides it
    low = (vol >> 4).astype(np.uint16)
    _, v12, _ = reslice_ref.render(rslib, low, geom, w, h, mode="mean", n=1024, filt=0, min_val=0, max_val=4095, u16_offset=False)
    s12, _ = mean_slab_samples(low, geom, w, h, 1024)
    assert np.array_equal(bits(v12), bits(s12.astype(np.float64).sum(axis=0).astype(np.float32) / np.float32(1024)))
