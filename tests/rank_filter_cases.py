"""TEST INFRASTRUCTURE ONLY -- the rank filter kernels (csrc/vr_rank.hip) at the limits their launcher has: the LDS ring of the
y and z passes, their column segments, the x pass's tiles and the median's tiles; for tests/test_rank_filter_cpu.py, which
proves that each case reaches what it is named for, and tests/test_rank_filter_gpu.py, which runs them against
tests/rank_ref/rank_ref.c bit for bit.

The host decides from the shape alone how many workgroups march along a column and in how many steps.  This module restates
that rule (rank_column_segment, csrc/rank_schedule.h) -- the CPU test holds the restatement to the C++ function itself, through
tests/rank_schedule/schedule_check.cpp -- and the kernels' constants.

Volumes are indexed [z, y, x]; shapes are (nx, ny, nz); radii are (rx, ry, rz).
"""
from collections import namedtuple

import numpy as np

MAX_RADIUS = 8                          # kRankMaxRadius
STEP = 16                               # rows a column workgroup computes per marching step
RING = 32                               # kRing: rows of the LDS ring, 16 + 2 * 8
X_TILE = 128                            # kXTile
MEDIAN_TILE = (64, 8, 8)                # kMedX, kMedY, kMedZ
MIN_WORKGROUPS = 2048                   # rank_column_segment stops halving a column once the grid has that many

OFF, ERODE, DILATE, OPEN, CLOSE, MEDIAN = range(6)
MORPHOLOGY = (ERODE, DILATE, OPEN, CLOSE)
OP_NAMES = {OFF: "off", ERODE: "erode", DILATE: "dilate", OPEN: "open", CLOSE: "close", MEDIAN: "median"}

# the issue's shapes and radii
SHAPES = [(13, 11, 6), (70, 66, 68), (5, 3, 1), (64, 1, 1), (129, 4, 4)]
MORPHOLOGY_RADII = [(1, 1, 1), (2, 0, 3), (8, 1, 0), (0, 0, 8)]
MEDIAN_RADII = [tuple(m >> a & 1 for a in range(3)) for m in range(1, 8)]


def _ceil16(n):
    return (n + 15) // 16 * 16


def column_segment(na, columns):
    """rank_column_segment (csrc/rank_schedule.h)"""
    seg = _ceil16(na)
    while seg > 64 and columns * -(-na // seg) < MIN_WORKGROUPS:
        seg = _ceil16(seg // 2)
    return seg


ColPlan = namedtuple("ColPlan", "columns seg segs steps last wraps")


def col_plan(shape, axis, r):
    """launch_minmax (csrc/vr_rank.hip) for the pass along axis 1 (y) or 2 (z): workgroups across the columns, outputs per
    workgroup, workgroups per column, marching steps of a whole segment, outputs of the last segment, and whether a workgroup's
    newest staged row (16 * step + 2r + 15) ever lies beyond the ring's last one, i.e. is written over the oldest"""
    nx, ny, nz = shape
    na, nb = (ny, nz) if axis == 1 else (nz, ny)
    columns = -(-nx // 64) * -(-nb // 4)
    seg = column_segment(na, columns)
    segs = -(-na // seg)
    steps = -(-min(seg, na) // STEP)
    return ColPlan(columns, seg, segs, steps, na - (segs - 1) * seg, STEP * (steps - 1) + 2 * r + STEP - 1 >= RING)


# name -> (shape, radii, the pass's axis): every case at the largest radius, where the ring is full (16 + 2 * 8 rows)
LIMIT_CASES = {
    "RING_FITS_Y": ((9, 16, 5), (0, 8, 0), 1),          # one step: the 32 rows fill the ring exactly, nothing is overwritten
    "RING_WRAPS_Y": ((9, 17, 5), (0, 8, 0), 1),         # a second step: its rows overwrite the first step's
    "RING_FITS_Z": ((9, 5, 16), (0, 0, 8), 2),
    "RING_WRAPS_Z": ((9, 5, 17), (0, 0, 8), 2),
    "ONE_SEGMENT_Y": ((9, 64, 5), (0, 8, 0), 1),        # the longest column that is never split
    "TWO_SEGMENTS_Y": ((9, 65, 5), (0, 8, 0), 1),       # seg 48: 48 + 17 outputs, the halo of each read from the other's rows
    "ONE_SEGMENT_Z": ((9, 5, 64), (0, 0, 8), 2),
    "TWO_SEGMENTS_Z": ((9, 5, 65), (0, 0, 8), 2),
    "FOUR_SEGMENTS_Z": ((10, 6, 200), (0, 0, 8), 2),    # seg 64, two interior segments, a last one of 8 outputs
    "SPLIT_BELOW_2048_Y": ((4, 65, 8188), (0, 8, 0), 1),    # 2047 columns: still split
    "WHOLE_FROM_2048_Y": ((4, 65, 8189), (0, 8, 0), 1),     # 2048 columns: one workgroup marches the whole column, five steps
}
# what col_plan must say of them: (seg, segs, steps, last, wraps)
LIMIT_PLANS = {
    "RING_FITS_Y": (16, 1, 1, 16, False), "RING_WRAPS_Y": (32, 1, 2, 17, True),
    "RING_FITS_Z": (16, 1, 1, 16, False), "RING_WRAPS_Z": (32, 1, 2, 17, True),
    "ONE_SEGMENT_Y": (64, 1, 4, 64, True), "TWO_SEGMENTS_Y": (48, 2, 3, 17, True),
    "ONE_SEGMENT_Z": (64, 1, 4, 64, True), "TWO_SEGMENTS_Z": (48, 2, 3, 17, True),
    "FOUR_SEGMENTS_Z": (64, 4, 4, 8, True),
    "SPLIT_BELOW_2048_Y": (48, 2, 3, 17, True), "WHOLE_FROM_2048_Y": (80, 1, 5, 65, True),
}
# tiles: the x pass's 128 outputs (a seam inside the radius-8 window on both sides), the median's 64 x 8 x 8
TILE_CASES = {
    "X_THREE_TILES": ((261, 9, 5), (8, 0, 0)),          # 128 + 128 + 5, a last quad of one voxel, unaligned rows
    "X_TWO_WHOLE_TILES": ((256, 5, 3), (8, 0, 0)),
    "MEDIAN_ONE_TILE": ((64, 8, 8), (1, 1, 1)),
    "MEDIAN_ONE_MORE": ((65, 9, 9), (1, 1, 1)),         # one voxel in the second tile along every axis
}


def peak(dtype):
    return 255 if np.dtype(dtype) == np.uint8 else 65535


def random_volume(shape, dtype, seed):
    """uniform over the whole range of the type"""
    nx, ny, nz = shape
    return np.random.default_rng(seed).integers(0, peak(dtype) + 1, size=(nz, ny, nx)).astype(dtype)


def extremes_volume(dtype):
    """33 x 32 x 31, random, with 0 and the maximum at opposite corners, a saturated corner block, and a band of the two values
    either side of the sign bit (127 | 128, 32767 | 32768): a signed compare orders those the wrong way round"""
    hi = peak(dtype)
    half = (hi + 1) // 2
    vol = random_volume((33, 32, 31), dtype, 12)
    vol[10:16] = np.where(np.random.default_rng(13).integers(0, 2, size=vol[10:16].shape) == 1, half, half - 1).astype(dtype)
    vol[0, 0, 0] = hi; vol[-1, -1, -1] = 0; vol[0, -1, 0] = 0; vol[-1, 0, -1] = hi
    vol[0:2, 0:2, -2:] = hi
    return vol


def few_values_volume(shape, dtype, n_values, seed):
    """only n_values distinct values, spread over the type's range (so that they also straddle the sign bit)"""
    hi = peak(dtype)
    values = np.asarray([0, hi] if n_values == 2 else [hi // 2, hi // 2 + 1, hi], dtype=dtype)
    nx, ny, nz = shape
    return values[np.random.default_rng(seed).integers(0, n_values, size=(nz, ny, nx))]
