"""TEST INFRASTRUCTURE ONLY -- 16-bit volumes over the whole value range, for tests/test_u16_full_range_{cpu,gpu}.py.

Three kinds.  `scaled`: 16 x a 12-bit field (the noise ball, a smooth field or uniform noise), so every voxel is a multiple of
16 up to 65520 and the volume has a 12-bit twin.  `white`: uniform in [0, 65536) with one voxel set to 0 and one to 65535.
`shifted`: a 12-bit field + B, so the range is at most 4095 wide (it packs) while every voxel lies above 4095.

The twins matter because two exact invariances tie a full-range frame to a 12-bit one: scaling the voxels and the window by 16
scales every fp32 operand by a power of two, and adding B to the voxels and the window leaves (float)(v + B) - (float)(lo + B)
exact (NEAREST only).
"""
from collections import namedtuple

import numpy as np

SCALE = 16
SHIFTS = (12345, 61440)
SCALED_KINDS = ("scaled_ball", "scaled_smooth", "scaled_rand")

# vol: the full-range volume; twin: its 12-bit twin (None for `white`); scale / shift: vol == scale * twin + shift
Volume = namedtuple("Volume", "kind vol twin scale shift")


def smooth12(rng, dims):
    """a smooth 12-bit field with a little noise on top (what the parity tests call a smooth volume)"""
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    v = ((np.sin(x * 0.3) + np.cos(y * 0.23) + np.sin(z * 0.31) + 3) / 6 * 4095).astype(np.int64)
    v += rng.integers(0, 3, size=v.shape)
    return np.clip(v, 0, 4095).astype(np.uint16)


def rand12(rng, dims):
    nx, ny, nz = dims
    return rng.integers(0, 4096, size=(nz, ny, nx)).astype(np.uint16)


def white16(rng, dims):
    nx, ny, nz = dims
    v = rng.integers(0, 65536, size=(nz, ny, nx)).astype(np.uint16)
    flat = v.reshape(-1)
    a, b = (int(i) for i in rng.choice(flat.size, size=2, replace=False))
    flat[a], flat[b] = 0, 65535
    return v


def twin12(oracle, rng, dims, field):
    if field == "ball":
        return oracle.gen_noise_ball(dims, 2, int(rng.integers(1 << 31)))
    return smooth12(rng, dims) if field == "smooth" else rand12(rng, dims)


def make(oracle, kind, dims, seed):
    """kind: scaled_ball | scaled_smooth | scaled_rand | white | shifted12345 | shifted61440"""
    rng = np.random.default_rng(seed)
    if kind == "white":
        out = Volume(kind, white16(rng, dims), None, 1, 0)
    elif kind.startswith("scaled_"):
        twin = twin12(oracle, rng, dims, kind[len("scaled_"):])
        out = Volume(kind, (twin.astype(np.uint32) * SCALE).astype(np.uint16), twin, SCALE, 0)
    elif kind.startswith("shifted"):
        shift = int(kind[len("shifted"):])
        twin = twin12(oracle, rng, dims, ("smooth", "ball", "rand")[seed % 3])
        out = Volume(kind, (twin.astype(np.uint32) + shift).astype(np.uint16), twin, 1, shift)
    else:
        raise ValueError(kind)
    check(out)
    return out


def check(v):
    """what every full-range case needs to be one: data above the 12-bit corner, and plenty of it"""
    vol = v.vol
    assert vol.dtype == np.uint16 and int(vol.max()) > 4095, v.kind
    if v.twin is not None:
        assert int(v.twin.max()) <= 4095
        assert np.array_equal(vol.astype(np.int64), v.twin.astype(np.int64) * v.scale + v.shift)
    if v.kind == "white":
        assert int(vol.min()) == 0 and int(vol.max()) == 65535
    if v.kind == "white" or v.kind.startswith("scaled_"):
        assert float((vol > 4095).mean()) >= 0.40, (v.kind, float((vol > 4095).mean()))
    if v.kind.startswith("shifted"):
        assert int(vol.max()) - int(vol.min()) <= 4095


def twin_window(v, lo, hi):
    """the stored-unit window of the twin's frame -> the window of the full-range frame that must equal it"""
    return v.scale * lo + v.shift, v.scale * hi + v.shift


MEAN_DIMS = (31, 22, 96)            # nx, ny, nz: 1024 samples over the 96 slices, every one of them inside


def mean_order_case(oracle):
    """shared with the GPU file: a `white` volume and an axial slab of 1024 samples, 3/32 voxel apart"""
    v = make(oracle, "white", MEAN_DIMS, 4242)
    nx, ny, nz = MEAN_DIMS
    geom = np.array([0, 0, (nz - 1) / 2.0, 1, 0, 0, 0, 1, 0, 0, 0, 3.0 / 32.0], dtype=np.float32)
    return v.vol, geom, (nx, ny)
