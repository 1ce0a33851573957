"""TEST INFRASTRUCTURE ONLY -- the switch between 32-bit and 64-bit voxel offsets, for tests/test_offset_limits_{cpu,gpu}.py.

Every kernel that reads the volume has two address paths, chosen per frame by RendererCore::buildFrame (csrc/renderer_core.cpp, the
`small` predicate behind LaunchConfig::big_offsets): 32-bit offsets built with 24-bit multiplies and fetched through a
bounds-checked buffer resource, or 64-bit offsets and plain global loads.  takes_32bit_path() restates that predicate; the shape
tables below are the volumes that sit on it -- one shape just inside each condition and its neighbour just outside, and the
smallest volumes whose 32-bit offsets have bit 31 set.

Volumes are indexed [z, y, x]; dims are (nx, ny, nz).
"""
from collections import namedtuple

import numpy as np

LINEAR, BRICKED = 0, 1
BRICK = 4                           # 4 x 4 x 4 voxels, 64 per brick (csrc/vr_frame.h)
LIM24, LIM32 = 1 << 24, 1 << 32


def bricks(n):
    return (n + BRICK - 1) // BRICK


def storage_voxels(dims, layout):
    """RendererCore::storageVoxels: the bricked layout stores whole bricks"""
    nx, ny, nz = dims
    return nx * ny * nz if layout == LINEAR else bricks(nx) * bricks(ny) * bricks(nz) * 64


def brick_strides(dims):
    """(bstride_y, bstride_z) of VoxelAddr<1, false>: the strides of a brick row and a brick layer in voxels, minus the part of
    the in-brick term the split axis repeats"""
    bnx, bny = bricks(dims[0]), bricks(dims[1])
    return 64 * bnx - BRICK * BRICK, 64 * bnx * bny - 64


def failed_conditions(dims, bytes_per_voxel, layout):
    """the conditions of the 32-bit path that the volume does not meet, by name; empty: the 32-bit path"""
    nx, ny, nz = dims
    storage = storage_voxels(dims, layout)
    out = []
    if not storage < LIM32:
        out.append("voxels")
    if not storage * bytes_per_voxel < LIM32:
        out.append("bytes")
    if not (nx < LIM24 and ny < LIM24 and nz < LIM24):
        out.append("dimension")
    if layout == LINEAR:
        if not ny * nz < LIM24:
            out.append("ny*nz")
    else:
        bsy, bsz = brick_strides(dims)
        if not bsy < LIM24:
            out.append("bstride_y")
        if not bsz < LIM24:
            out.append("bstride_z")
    return out


def takes_32bit_path(dims, bytes_per_voxel, layout):
    return not failed_conditions(dims, bytes_per_voxel, layout)


def highest_offset(dims, layout):
    """the element offset of the last voxel (nx - 1, ny - 1, nz - 1)"""
    nx, ny, nz = dims
    if layout == LINEAR:
        return nx * ny * nz - 1
    i, j, k = nx - 1, ny - 1, nz - 1
    brick = (i // 4) + bricks(nx) * ((j // 4) + bricks(ny) * (k // 4))
    return brick * 64 + (i % 4) + 4 * (j % 4) + 16 * (k % 4)


# ---------------------------------------------------------------------------------------------------------------
# 1: one shape just inside each stride condition and its neighbour just outside
# ---------------------------------------------------------------------------------------------------------------
# inside / outside: dims on the 32-bit / the 64-bit side; spacing: one that makes the box of the flat volumes 1 x 1 x 0.25 (or
# 0.25 x 1 x 1); rays: whether camera rays cross the volume usefully (the lines of voxels are longer than the 10 000-step cap)
Threshold = namedtuple("Threshold", "name layout inside outside spacing rays")
THRESHOLDS = {
    t.name: t for t in (
        Threshold("bstride_z", BRICKED, (2048, 2048, 8), (2052, 2048, 8), (1.0, 1.0, 64.0), True),        # bstride_z = 2^24 - 64 | 2^24 + 32704
        Threshold("ny*nz", LINEAR, (4, 4096, 4095), (4, 4096, 4096), (256.0, 1.0, 1.0), True),            # ny * nz = 2^24 - 4096 | 2^24
        Threshold("bstride_y", BRICKED, (1048576, 4, 4), (1048580, 4, 4), (1.0, 1.0, 1.0), False),        # bstride_y = 2^24 - 16 | 2^24 + 48
        Threshold("dimension", LINEAR, (16777215, 1, 1), (16777216, 1, 1), (1.0, 1.0, 1.0), False),       # nx = 2^24 - 1 | 2^24
    )
}

# ---------------------------------------------------------------------------------------------------------------
# 2: the 32-bit path with bit 31 of the offset set
# ---------------------------------------------------------------------------------------------------------------
# layouts: the layouts the volume is rendered in; beyond: the shape just beyond it, which is 64-bit in every layout (None: the
# volume is not at the top of the path)
BigVolume = namedtuple("BigVolume", "name dims bytes_per_voxel layouts beyond")
BIG_VOLUMES = {
    v.name: v for v in (
        BigVolume("u16_2gib", (1024, 1024, 1032), 2, (BRICKED, LINEAR), None),              # byte offsets >= 2^31 through off << 1
        BigVolume("u8_2gib", (2048, 2048, 520), 1, (BRICKED, LINEAR), None),                # element offsets >= 2^31; bricked: bstride_z at its maximum
        BigVolume("u8_4gib", (2048, 2048, 1020), 1, (BRICKED,), (2048, 2048, 1024)),        # 4 278 190 080 bytes: the top of the path
        BigVolume("u16_4gib", (1024, 2048, 1020), 2, (LINEAR,), (1024, 2048, 1024)),
    )
}


def first_plane_with_bit31(dims, bytes_per_voxel, layout):
    """the first z plane that holds a voxel whose storage offset in BYTES (16-bit) or ELEMENTS (8-bit) reaches 2^31"""
    nx, ny, nz = dims
    limit = (1 << 31) // bytes_per_voxel                    # in elements
    if layout == LINEAR:
        k = limit // (nx * ny)                              # the plane of element `limit`
    else:
        k = (limit // (bricks(nx) * bricks(ny) * 64)) * 4   # the brick layer of element `limit` starts here
    assert 0 < k < nz, (dims, k)
    return k


def rand_voxels(rng, dims, dtype):
    """uniform voxels over the range tests/test_parity_gpu.py::rand_volume draws from (8 bits / 12 bits), generated in the
    voxel type (the volumes here have up to 2^26 voxels)"""
    nx, ny, nz = dims
    return rng.integers(0, 256 if np.dtype(dtype) == np.uint8 else 4096, size=(nz, ny, nx), dtype=dtype)


def clear_first_corner(vol):
    """zeroes the quarter of the volume next to voxel (0, 0, 0) along every axis of 64 voxels or more: cells that empty-space
    skipping can skip, far from the last voxel"""
    nz, ny, nx = vol.shape
    sl = tuple(slice(0, n // 4) if n >= 64 else slice(None) for n in (nz, ny, nx))
    vol[sl] = 0
    return vol


def corner_camera(E, dims, spacing, view, dist=0.03, view_plane_dist=4.0):
    """A camera outside the box that looks at the centre of the last voxel (nx - 1, ny - 1, nz - 1) along the box's diagonal: the
    rays through the middle of the image enter at that voxel and cross the volume to voxel (0, 0, 0).  E: tests/edge_cases.py"""
    target = E.voxel_centre_in_box(dims, spacing, view, tuple(n - 1 for n in dims))
    out = np.sign(target) * np.array([0.6, 0.5, 0.62])
    out /= np.linalg.norm(out)
    eye = target + dist * out
    look = -out
    side = np.cross(look, np.array([0.0, 1.0, 0.0])); side /= np.linalg.norm(side)
    up = np.cross(side, look)
    b = np.zeros(21, dtype=np.float32)
    b[0:3] = side; b[4:7] = up; b[8:11] = -look; b[12:15] = eye; b[15] = 1
    b[16:19] = eye; b[19] = 1
    b[20] = view_plane_dist
    return b
