"""The intended side of every threshold between 32-bit and 64-bit voxel offsets, as a record: tests/offset_limits.py restates
RendererCore::buildFrame's predicate (csrc/renderer_core.cpp: `small`), and the shapes tests/test_offset_limits_gpu.py renders are
pinned to their side here, each with the one condition that puts it there.  No GPU."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

_spec = importlib.util.spec_from_file_location("offset_limits", Path(__file__).resolve().parent / "offset_limits.py")
O = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(O)


@pytest.mark.parametrize("name", list(O.THRESHOLDS))
def test_each_threshold_has_a_shape_on_either_side(name):
    """the inside shape meets every condition; its neighbour fails the named one and no other, for 8-bit and 16-bit voxels
    (one brick more along x of a volume one brick high takes bstride_z = bstride_y + 16 - 64 over the limit with bstride_y)"""
    t = O.THRESHOLDS[name]
    want = ["bstride_y", "bstride_z"] if name == "bstride_y" else [name]
    for b in (1, 2):
        assert O.failed_conditions(t.inside, b, t.layout) == [], (name, b)
        assert O.failed_conditions(t.outside, b, t.layout) == want, (name, b)
        assert O.storage_voxels(t.outside, t.layout) * b <= 128 << 20           # seconds on a GPU, not minutes


def test_the_inside_shapes_sit_on_the_limit():
    """the factor in question is the largest the 24-bit multiplies may see, or one step (a brick of x, a row of z) below it"""
    t = O.THRESHOLDS
    assert O.brick_strides(t["bstride_z"].inside)[1] == (1 << 24) - 64 and O.brick_strides(t["bstride_z"].outside)[1] >= 1 << 24
    assert O.brick_strides(t["bstride_y"].inside)[0] == (1 << 24) - 16 and O.brick_strides(t["bstride_y"].outside)[0] >= 1 << 24
    nx, ny, nz = t["ny*nz"].inside
    assert ny * nz == (1 << 24) - ny and (nz - 1) * ny + ny - 1 < 1 << 24       # the largest row index k * ny + j
    assert t["ny*nz"].outside[1] * t["ny*nz"].outside[2] == 1 << 24
    assert t["dimension"].inside[0] == (1 << 24) - 1 and t["dimension"].outside[0] == 1 << 24
    # the other layout of the flat volumes is not at a limit: the threshold belongs to the layout the table names
    assert O.takes_32bit_path(t["ny*nz"].outside, 2, O.BRICKED)
    assert O.takes_32bit_path(t["bstride_z"].outside, 2, O.LINEAR)


@pytest.mark.parametrize("name", list(O.BIG_VOLUMES))
def test_big_volumes_are_32bit_with_bit_31_set(name):
    v = O.BIG_VOLUMES[name]
    for layout in v.layouts:
        assert O.takes_32bit_path(v.dims, v.bytes_per_voxel, layout), (name, layout)
        top = O.highest_offset(v.dims, layout)
        assert top < 1 << 32 and top * v.bytes_per_voxel >= 1 << 31, (name, layout, top)
        if v.bytes_per_voxel == 1:
            assert top >= 1 << 31                                               # the element offset itself
        k = O.first_plane_with_bit31(v.dims, v.bytes_per_voxel, layout)
        assert 4 <= k < v.dims[2] - 4, (name, layout, k)                        # planes on either side of it exist
    assert sum(v.dims) > 3072                                                   # no address tables below 2^32, no packed copy
    if v.beyond is not None:
        for layout in (O.LINEAR, O.BRICKED):
            failed = O.failed_conditions(v.beyond, v.bytes_per_voxel, layout)
            assert "bytes" in failed, (name, layout, failed)
        assert O.storage_voxels(v.dims, v.layouts[0]) * v.bytes_per_voxel == 4278190080


def test_first_plane_with_bit31_is_the_first():
    """against a direct search over the planes' lowest and highest element offsets"""
    for v in O.BIG_VOLUMES.values():
        nx, ny, nz = v.dims
        for layout in v.layouts:
            limit = (1 << 31) // v.bytes_per_voxel
            if layout == O.LINEAR:
                highest = [(k + 1) * nx * ny - 1 for k in range(nz)]
            else:
                layer = O.bricks(nx) * O.bricks(ny) * 64
                highest = [(k // 4 + 1) * layer - 1 - 16 * (3 - k % 4) for k in range(nz)]
            first = next(k for k in range(nz) if highest[k] >= limit)
            assert first == O.first_plane_with_bit31(v.dims, v.bytes_per_voxel, layout), (v.name, layout)


def test_highest_offset_matches_a_brute_force_relayout():
    rng = np.random.default_rng(5)
    for dims in ((5, 7, 9), (8, 4, 4), (1, 1, 1), (13, 2, 6)):
        nx, ny, nz = dims
        offs = set()
        for k in range(nz):
            for j in range(ny):
                for i in range(nx):
                    brick = (i // 4) + O.bricks(nx) * ((j // 4) + O.bricks(ny) * (k // 4))
                    offs.add(brick * 64 + (i % 4) + 4 * (j % 4) + 16 * (k % 4))
        assert len(offs) == nx * ny * nz and max(offs) < O.storage_voxels(dims, O.BRICKED)
        assert O.highest_offset(dims, O.BRICKED) == max(offs)
        assert O.highest_offset(dims, O.LINEAR) == nx * ny * nz - 1
    del rng
