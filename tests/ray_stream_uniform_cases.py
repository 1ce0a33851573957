"""TEST INFRASTRUCTURE ONLY -- wavefronts whose lanes part ways in the replay loop of the ray-ordered sample stream
(csrc/vr_stream.hip), for
tests/test_ray_stream_uniform_cpu.py and tests/test_ray_stream_uniform_gpu.py.  Geometry, cameras, modes and the size models
are tests/ray_stream_cases.py's (S) and tests/ray_stream_pack_cases.py's (C); here is a model of how long a wavefront stays
uniform and the cases that steer it.

A lane loads its samples in units of one group (8 samples packed, 4 unpacked) and composites them four at a time, skipping
the per-sample tests of four samples that lie inside its n with dest.a < 0.95 before the last of them.  A unit is called fast
here while (a) every lane of the wavefront has the whole unit inside its n and (b) dest.a < 0.95 holds before the unit's last
sample in every lane: every lane skips the tests and the wavefront runs undiverged.  In the first unit that fails either, and
in the units after it, lanes run the literal per-sample tests, end or are dead beside live ones.  From the oracle's per-pixel
sample counts -- n (geometric, alpha_scale 0) and spp (composited) -- both are known per stream block: fast_units() below.

Volumes are indexed [z, y, x]; sizes are (width, height).
"""
import importlib.util
from pathlib import Path

import numpy as np

_spec = importlib.util.spec_from_file_location("ray_stream_pack_cases", Path(__file__).resolve().parent / "ray_stream_pack_cases.py")
C = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(C)
S = C.S

STREAM, STREAM12 = S.STREAM, C.STREAM12
DIMS = S.RESIDUE_DIMS
SIZE = S.RESIDUE_SIZE                    # 96 x 80: 120 stream blocks
HELD = 8                                 # 2 * VR_STREAM_DEPTH = 2 * VR_STREAM12_DEPTH: loaded groups a wavefront holds (cur and nxt)
UNITS = {"packed": C.G12, "unpacked": S.G}
EDGE_POSE = S.RESIDUE_POSES[1]
CLOSE_POSE = S.CLOSE_POSE


def lanes(a):
    """a per-pixel array over the launch's local rows as [blocks, 64]: the 64 lanes of every 8 x 8 stream block, 0 outside"""
    h, w = a.shape
    g = S.stream_grid(w, h)
    p = np.zeros((g.blocks_y * 8, g.blocks_x * 8), dtype=np.int64)
    p[:h, :w] = a
    return p.reshape(g.blocks_y, 8, g.blocks_x, 8).transpose(0, 2, 1, 3).reshape(g.blocks, 64)


def fast_units(n, spp, unit):
    """per block: (fast units, units of the block).  A lane ended by opacity (spp < n) had dest.a >= 0.95 before
    sample index spp, so the first unit whose last sample index u * unit + unit - 1 >= spp fails (b): u = spp // unit; (a) holds
    for u < min n // unit"""
    ln, ls = lanes(n), lanes(spp)
    by_length = ln.min(axis=1) // unit
    early = (ln > 0) & (ls < ln)
    by_opacity = np.where(early, ls // unit, np.iinfo(np.int64).max).min(axis=1)
    return np.minimum(by_length, by_opacity), (ln.max(axis=1) + unit - 1) // unit


# ---------------------------------------------------------------------------------------------------------------
# U1: opacity ends rays at different samples inside one wavefront
# ---------------------------------------------------------------------------------------------------------------
# Every voxel column along z holds one value; the front-facing poses march (nearly) along z, so a ray sees (nearly) one value
# v, a = v / max per sample at alpha 1, and ends after about k samples where (1 - a)^k <= 0.05.  k is drawn per column from
# 8 .. 40, so neighbouring pixels end in different units of eight and at every residue.
RAMP_K = (8, 41)
RAMP_MIN_BLOCKS = 8


def ramp_volume(kind):
    top = 4095 if kind == "u16" else 255
    k = np.random.default_rng(11).integers(*RAMP_K, size=DIMS[1::-1])
    a = 1.0 - 0.05 ** (1.0 / (k - 0.5))
    v = np.round(a * top).astype(np.uint16 if kind == "u16" else np.uint8)
    return np.ascontiguousarray(np.broadcast_to(v[None], DIMS[::-1]))


def ramp_window(kind):
    return (0, 4095) if kind == "u16" else (0, 255)


def scattered_end_blocks(n, spp):
    """blocks whose lanes ended by opacity fall into three or more different units of eight and cover all eight residues"""
    ln, ls = lanes(n), lanes(spp)
    count = 0
    for b in range(ln.shape[0]):
        e = ls[b][(ln[b] > 0) & (ls[b] < ln[b])]
        count += int(len(e) > 0 and len(np.unique(e // 8)) >= 3 and len(np.unique(e % 8)) == 8)
    return count


# ---------------------------------------------------------------------------------------------------------------
# U2: wavefronts whose 64 rays have one n -- fast units only, until their last unit
# ---------------------------------------------------------------------------------------------------------------
# The 64^3 volume as a slab: spacing z makes the box `z` thick, and from the close pose (every pixel hits) the blocks near the
# image centre have 64 rays of one length.  z -> that n: 16 = two whole units of eight (the last unit is fast too), 8 one, and
# 9 .. 15 one whole unit and a last, literal one with 1 .. 7 samples.
SLAB_Z = {8: 0.09, 9: 0.105, 10: 0.115, 11: 0.13, 12: 0.14, 13: 0.155, 14: 0.17, 15: 0.18, 16: 0.195}
SLAB_MIN_BLOCKS = 8
SLAB_ALPHA = 0.02


def slab_spacing(n):
    return (1.0, 1.0, SLAB_Z[n])


def equal_blocks(n, value):
    """blocks whose 64 lanes all have n == value"""
    ln = lanes(n)
    return int(np.count_nonzero((ln.min(axis=1) == value) & (ln.max(axis=1) == value)))


# ---------------------------------------------------------------------------------------------------------------
# U3: mixed wavefronts
# ---------------------------------------------------------------------------------------------------------------
# Lanes of n = 0 beside live lanes: the edge pose (its silhouette crosses 30 blocks).  Exactly one lane at least eight samples
# shorter than the other 63 -- and itself at least eight long, so the block starts with fast units -- needs a silhouette edge
# that cuts one corner pixel off a block: neither the edge pose nor the other two poses of tests/ray_stream_cases.py has such a
# block at any of 96 x 80, 328 x 264 and 600 x 456 (the CPU file asserts it for 96 x 80), so a rolled camera is used whose
# silhouette runs diagonally through the block grid (found by a seeded random search over look_block cameras).
MIXED_MIN_BLOCKS = 8
ROLLED_CAMERA = ((-2.362, -0.25, -0.59), (2.672, 0.211, 0.656), 4.0, (2.087, -0.575, -0.235))     # eye, look, view plane, up hint


def rolled_camera():
    eye, look, dist, up = ROLLED_CAMERA
    return S.look_block(eye, look, dist, up)


def dead_beside_live_blocks(n):
    ln = lanes(n)
    return int(np.count_nonzero((ln.min(axis=1) == 0) & (ln.max(axis=1) > 0)))


def one_short_lane_blocks(n, by=8):
    ln = np.sort(lanes(n), axis=1)
    return int(np.count_nonzero((ln[:, 0] >= by) & (ln[:, 0] + by <= ln[:, 1])))


# ---------------------------------------------------------------------------------------------------------------
# U4: every mode on the new path (the close pose: every block has fast units)
# ---------------------------------------------------------------------------------------------------------------
# (name, volume, window, mode): the arithmetic classification with the clamp (the window cuts into the data) and without it (the
# window contains the data), with the shifted window (base 1000) and with the integer add (a window limit of 2^24), then the
# table modes
MODE_CASES = [
    ("grey_noclamp", "ball", (0, 4095), "grey"),
    ("grey_clamp", "ball", (500, 3000), "grey"),
    ("grey_shifted_noclamp", "offset", (900, 5200), "grey"),
    ("grey_shifted_clamp", "offset", (2000, 4000), "grey"),
    ("grey_baseadd", "offset", (0, 1 << 24), "grey"),
    ("mip_baseadd", "offset", (0, 1 << 24), "mip"),
    ("grey_tf", "ball", (0, 4095), "grey_tf"),
    ("mip", "ball", (0, 4095), "mip"),
    ("tf", "ball", (0, 4095), "tf"),
    ("mip_tf", "ball", (0, 4095), "mip_tf"),
]
MODE_ALPHAS = (0.02, 1.0)


def mode_volume(oracle, name):
    return S.residue_volume(oracle, "u16") if name == "ball" else C.offset_volume(oracle)


# ---------------------------------------------------------------------------------------------------------------
# U5: addressing
# ---------------------------------------------------------------------------------------------------------------
def block_groups(n, fmt):
    """groups of every block in stream order"""
    return (lanes(n).max(axis=1) + UNITS[fmt] - 1) // UNITS[fmt]


def odd_start_blocks(n):
    """packed blocks with samples whose first byte is an odd multiple of 768 into the stream"""
    g = block_groups(n, "packed")
    starts = np.concatenate(([0], np.cumsum(g)[:-1]))
    return int(np.count_nonzero((g > 0) & (starts % 2 == 1)))
