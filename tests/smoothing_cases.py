"""TEST INFRASTRUCTURE ONLY -- Gaussian smoothing (csrc/vr_smooth.hip, RendererCore::smoothPasses) at the limits of its LDS ring,
its column segments, its x tiles and its z slabs, for tests/test_smoothing_cases_cpu.py and tests/test_smoothing_edges_gpu.py.

Which kernel instance runs, with which ring, over how many segments of how many marching steps, across how many x tiles and in
how many slabs is decided on the host from the shape, the radii and the workspace.  This module restates those rules -- the
radius, launch_col's segment and ring, smoothPasses' slab -- and holds the shapes and sigmas chosen with them.  The CPU file
proves that each case reaches what it is named for and that no shape of tests/test_smoothing_gpu.py does; the GPU file runs
them against tests/smooth_ref/smooth_ref.c bit for bit.  The library reports neither the segment nor the ring, so the two plan
functions cannot be checked against it: that they describe it was shown by planted errors (docs/lab-notebook.md).

Volumes are indexed [z, y, x]; shapes are (nx, ny, nz); sigmas are (x, y, z) in voxels.
"""
import math
from collections import namedtuple

import numpy as np

MAX_RADIUS = 24                         # kSmoothMaxRadius
STEP = 16                               # rows a column workgroup computes per marching step
X_TILE = 128                            # kXTile: outputs along x per workgroup of the x pass
MIN_WORKGROUPS = 2048                   # launch_col stops halving a column once the grid has that many


# ---------------------------------------------------------------------------------------------------------------
# the host's rules, restated
# ---------------------------------------------------------------------------------------------------------------
def radius(sigma):
    """smooth_weights (csrc/vr_smooth.hip): r = ceil(3 sigma) of the fp32 value the C ABI receives, at most 24"""
    return min(MAX_RADIUS, math.ceil(3.0 * float(np.float32(sigma))))


def sweep_sigma(r):
    """a sigma whose radius is r, for r = 1 .. 24"""
    return (r - 0.5) / 3.0


ColPlan = namedtuple("ColPlan", "ring seg segs steps last")


def _ceil16(n):
    return (n + 15) // 16 * 16


def col_plan(nx, nb, na, r):
    """launch_col (csrc/vr_smooth.hip): a column pass over `na` outputs along its axis and `nb` rows across it.  y pass: nb = the
    planes the pass covers, na = ny; z pass: nb = ny, na = the output planes.  ring: rows of the LDS ring; seg: outputs per
    workgroup; segs: workgroups per column; steps: marching steps of a whole segment; last: outputs of the last segment."""
    tiles = -(-nx // 64) * -(-nb // 4)
    seg = _ceil16(na)
    while seg > 64 and tiles * -(-na // seg) < MIN_WORKGROUPS:
        seg = _ceil16(seg // 2)
    ring = 32 if STEP + 2 * r <= 32 else 64
    segs = -(-na // seg)
    return ColPlan(ring, seg, segs, seg // STEP, na - (segs - 1) * seg)


def first_wrapping_step(r, ring):
    """smooth_col_kernel: the first step (from 0) whose newest staged row base + 2r + 15, base = 16 * step, is beyond the ring's
    last row, i.e. is written over the oldest one"""
    step = 0
    while STEP * step + 2 * r + STEP - 1 < ring:
        step += 1
    return step


def x_tiles(nx):
    """launch_x: workgroups along x"""
    return -(-nx // X_TILE)


SlabPlan = namedtuple("SlabPlan", "planes slab")


def slab_plan(nx, ny, nz, r_z, workspace_bytes):
    """RendererCore::smoothPasses (csrc/volume_ops.cpp), for a call with two or three passes and an explicit workspace bound:
    the fp32 planes one buffer holds and the output planes per slab; None where the call is refused (VR_E_NOMEM).  r_z = 0
    without a z pass."""
    planes = min(workspace_bytes // (nx * ny * 4), nz)
    if planes < min(nz, 2 * r_z + 1):
        return None
    return SlabPlan(planes, nz if planes >= nz else planes - 2 * r_z)


def slab_ranges(nz, r_z, slab):
    """(s0, s1, e0, e1) of every slab: output planes [s0, s1), planes the passes before z cover [e0, e1)"""
    return [(s0, min(s0 + slab, nz), max(s0 - r_z, 0), min(min(s0 + slab, nz) + r_z, nz)) for s0 in range(0, nz, slab)]


def instances(sig):
    """the kernel instances a sigma triple runs, as (axis, input, output) with "v" = voxels and "f" = fp32 planes: the order is
    x, y, z over the axes with sigma > 0; the first pass reads voxels, the last writes them (launch_smooth_type)"""
    axes = [a for a in range(3) if sig[a] > 0]
    return {("xyz"[a], "v" if k == 0 else "f", "v" if k == len(axes) - 1 else "f") for k, a in enumerate(axes)}


ALL_INSTANCES = {("x", "v", "v"), ("x", "v", "f"), ("y", "v", "v"), ("y", "v", "f"), ("y", "f", "v"), ("y", "f", "f"),
                 ("z", "v", "v"), ("z", "f", "v")}


# ---------------------------------------------------------------------------------------------------------------
# sigmas
# ---------------------------------------------------------------------------------------------------------------
# radius -> sigma: 8 fills RING = 32 (16 + 2 * 8 rows), 9 is the first radius of RING = 64, 24 fills RING = 64 (16 + 48)
RING_SIGMAS = {8: 2.5, 9: 3.0, 24: 8.0}


def SUBSETS(R):
    """sigma R on every non-empty subset of the axes, 0 on the rest.  The instances they run:
        (R, 0, 0)  x v->v            (0, R, 0)  y v->v            (0, 0, R)  z v->v
        (R, R, 0)  x v->f, y f->v    (R, 0, R)  x v->f, z f->v    (0, R, R)  y v->f, z f->v
        (R, R, R)  x v->f, y f->f, z f->v
    -- between them every instance launch_smooth_type knows"""
    return [tuple(R if m >> a & 1 else 0.0 for a in range(3)) for m in range(1, 8)]


MIXED = [(8.0, 2.5, 3.0), (3.0, 8.0, 2.5), (2.5, 3.0, 8.0)]

# ---------------------------------------------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------------------------------------------
SHAPES = {
    "COL_Z": (10, 6, 200),          # z pass: seg 64, 4 segments (two of them interior), 4 steps, a last segment of 8 outputs
    "COL_Y": (10, 200, 6),          # the same on the y pass
    "BOTH": (21, 150, 150),         # y and z: seg 48, 4 segments, 3 steps, a last segment of 6; 38 tiles: the split stops at seg <= 64
    "XT": (261, 9, 5),              # three x tiles (128 + 128 + 5), a last quad of one voxel, ny and nz no multiple of 4, unaligned rows
    "XT_ALIGNED": (256, 5, 3),      # two whole x tiles: vector stores on both sides of the seam
    "XT_EDGE": (129, 4, 4),         # one voxel in the second tile: its staged row is almost all halo and clamp
    "THIN": (12, 10, 30),           # nz < 2 * 24 + 1
    "SWEEP": (37, 35, 33),          # every radius; columns longer than one step, in one segment
}
# the plans of the whole-volume passes: name -> (y pass, z pass) as (seg, segs, steps, last)
COLUMN_PLANS = {
    "COL_Z": (None, (64, 4, 4, 8)),
    "COL_Y": ((64, 4, 4, 8), None),
    "BOTH": ((48, 4, 3, 6), (48, 4, 3, 6)),
}
# the voxels of XT whose radius-24 neighbourhood crosses a tile seam (x = 128, x = 256): a failure there names the seam
XT_SEAM_COLUMNS = (slice(104, 152), slice(232, 261))
X_SIGMAS = (0.5, 2.5, 8.0)

# E4: BOTH in z slabs.  (sigma, planes of workspace) -> output planes per slab
SLAB_CASES = [
    ((8.0, 8.0, 8.0), 49, 1),       # a slab is its halo and one output plane: 150 slabs
    ((8.0, 8.0, 8.0), 50, 2),
    ((8.0, 8.0, 8.0), 65, 17),      # the slab seams fall inside 16-row steps
    ((0.0, 8.0, 8.0), 49, 1),       # one workspace buffer; y writes the fp32 planes
    ((8.0, 3.0, 0.0), 1, 1),        # no z pass: a slab without a halo
]
THIN_SIGMA = (1.0, 1.0, 8.0)
THIN_PLANES_OK, THIN_PLANES_REFUSED = 30, 29
WORKSPACE_SLACK = 17                # bytes beyond whole planes, as in tests/test_smoothing_gpu.py


def workspace_bytes(shape, planes):
    return planes * shape[0] * shape[1] * 4 + WORKSPACE_SLACK


# ---------------------------------------------------------------------------------------------------------------
# volumes
# ---------------------------------------------------------------------------------------------------------------
def peak(dtype):
    return 255 if np.dtype(dtype) == np.uint8 else 65535


def random_volume(name, dtype):
    """uniform over the whole range of the type; one fixed volume per shape and type"""
    nx, ny, nz = SHAPES[name]
    seed = 1000 + sorted(SHAPES).index(name)
    return np.random.default_rng(seed).integers(0, peak(dtype) + 1, size=(nz, ny, nx)).astype(dtype)


VALUE_CASES = ("checkerboard", "corners", "centre", "origin")


def value_volume(kind, dtype, shape=None):
    """E5's volumes on BOTH's shape: a 0 / maximum checkerboard; the maximum with one zero voxel at each of the eight corners;
    zero with a single maximum voxel at the centre or at (0, 0, 0)"""
    nx, ny, nz = shape or SHAPES["BOTH"]
    hi = peak(dtype)
    if kind == "checkerboard":
        z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        return (((x + y + z) & 1) * hi).astype(dtype)
    if kind == "corners":
        vol = np.full((nz, ny, nx), hi, dtype=dtype)
        for k in (0, -1):
            for j in (0, -1):
                for i in (0, -1):
                    vol[k, j, i] = 0
        return vol
    vol = np.zeros((nz, ny, nx), dtype=dtype)
    if kind == "centre":
        vol[nz // 2, ny // 2, nx // 2] = hi
    elif kind == "origin":
        vol[0, 0, 0] = hi
    else:
        raise ValueError(kind)
    return vol
