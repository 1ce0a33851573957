"""TEST INFRASTRUCTURE ONLY -- the hybrid classification of the ray stream's replay loop (csrc/vr_stream.hip: TSHARE;
vr_set_ray_stream_table), for tests/test_ray_stream_table_cpu.py and tests/test_ray_stream_table_gpu.py.  Geometry, cameras,
modes and size models are tests/ray_stream_cases.py's (S), tests/ray_stream_pack_cases.py's (C) and
tests/ray_stream_uniform_cases.py's (U).

Of every four samples a lane composites, those at fixed positions are classified through an LDS table of the window's entries,
the others arithmetically.  What can go wrong is a table sample that differs from the arithmetic one -- a wrong entry, a clamp
missing on one side, the packed format's base folded wrongly -- or samples taken out of order.  A frame shows it only if such a
sample lands at a position of the other kind next to it, so the cases below put clamped samples, the window's first and last
entry and the rays' ends at every position of a group; the CPU file proves that they do.

Where a sample of a given kind sits on a ray is read from the oracle alone: an indicator volume (255 where the voxel has the
property, 0 elsewhere) rendered at alpha 1 under the window (0, 255) ends a ray right after the first such sample (a = 1, dest.a
= 1 >= 0.95), so its per-pixel sample count minus one is that sample's index.

Volumes are indexed [z, y, x]; sizes are (width, height).
"""
import importlib.util
from pathlib import Path

import numpy as np

_spec = importlib.util.spec_from_file_location("ray_stream_uniform_cases", Path(__file__).resolve().parent / "ray_stream_uniform_cases.py")
U = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(U)
C, S = U.C, U.S

STREAM, STREAM12 = S.STREAM, C.STREAM12
DIMS = S.RESIDUE_DIMS
SIZE = S.RESIDUE_SIZE                    # 96 x 80: 3 x 5 workgroup tiles, 120 stream blocks
TABLE_MAX = 4096                         # kStreamTableMax == FAST_LUT_MAX: entries of the table
TABLE_MIN_BYTES = 256 << 20              # kStreamTableMinBytes: the automatic mode takes the hybrid above it
SHARE = 4                                # VR_STREAM_TSHARE: table samples per four
TABLE_WG = 256                           # VR_STREAM_TWG: threads that share one table
POSITIONS = {1: (3,), 2: (1, 3), 4: (0, 1, 2, 3)}       # table_pos of vr_stream.hip: positions inside a group of four
MIN_RAYS = 20                            # rays asked of every residue
EDGE_POSE, CLOSE_POSE = U.EDGE_POSE, U.CLOSE_POSE
FAR_POSE = ((-1.0, 0.0, 0.0),)           # dollied out one unit: the box covers the middle of the image, the outer workgroups are empty
OFFSET_BASE = C.OFFSET_BASE


def extremes_volume(oracle):
    """the 12-bit noise ball with 0, 4095, 1000 and 3000 alternating in its central 16^3 voxels (shifted by one per row and by two
    per slice): the exact range is [0, 4095], a span of exactly 4095, and the ends of the range and of the window (1000, 3000)
    are values that rays through the centre read"""
    vol = oracle.gen_noise_ball(DIMS, 2, 0x5678).astype(np.uint16) & 0xFFF
    z, y, x = np.indices((16, 16, 16))
    vol[24:40, 24:40, 24:40] = np.array([0, 4095, 1000, 3000], dtype=np.uint16)[(x + y + 2 * z) % 4]
    return vol


def offset_extremes_volume(oracle):
    """the same, offset like CT data: range [1000, 5095], so the packed stream's base is 1000"""
    return (extremes_volume(oracle) + OFFSET_BASE).astype(np.uint16)


def volume(oracle, name):
    return {"extremes": extremes_volume, "offset": offset_extremes_volume}[name](oracle)


# (name, volume, window, mode, the packed stream takes the hybrid under mode 2, the unpacked stream does)
CASES = [
    ("window_is_the_range", "extremes", (0, 4095), "grey", True, True),            # NOCLAMP, TABLE_MAX entries, the last one read
    ("one_entry_more", "extremes", (0, 4096), "grey", False, False),               # 4097 entries: arithmetic
    ("window_inside", "extremes", (1000, 3000), "grey", True, True),                # clamps on both sides
    ("offset_window_is_the_range", "offset", (1000, 5095), "grey", True, True),    # base 1000 folded into the table's bias
    ("offset_window_inside", "offset", (2000, 4000), "grey", True, True),
    ("beyond_2_24", "offset", (0, 1 << 24), "grey", False, False),                 # the integer add (BASEADD); too wide anyway
    ("mip_beyond_2_24", "offset", (0, 1 << 24), "mip", False, False),
    ("mip", "extremes", (0, 4095), "mip", True, True),
    ("mip_window_inside", "offset", (2000, 4000), "mip", True, True),
    ("grey_tf", "extremes", (0, 4095), "grey_tf", False, False),                   # classified through its own table already
    ("tf", "extremes", (0, 4095), "tf", False, False),
]
CASE_ALPHAS = (0.02, 1.0)


def eligible(window, mode, packed, base=0):
    """streamTableEligible (csrc/vr_stream.h), restated"""
    lim = (1 << 24) - (1 << 17)
    entries = window[1] - window[0] + 1
    folds = 0 <= base < (1 << 16) and -lim < window[0] < lim and -lim < window[1] < lim
    return mode in ("grey", "mip") and 1 <= entries <= TABLE_MAX and (not packed or folds)


def first_index(oracle, mask, cam, size=SIZE, n=None):
    """per pixel: the index of the ray's first sample whose voxel lies in `mask`, -1 where it has none before its last sample
    (n: the geometric counts, if the caller has them)"""
    ind = np.where(mask, 255, 0).astype(np.uint8)
    if n is None:
        n = S.geometric_counts(oracle, ind, size, cam)
    spp = oracle.render(ind, S.params(oracle, size, cam, 1.0, (0, 255)), want_spp=True)[2]
    return np.where((n > 0) & (spp < n), spp.astype(np.int64) - 1, -1)


def residues(idx, modulus=S.G):
    """rays per residue of a first_index result"""
    return np.bincount(idx[idx >= 0] % modulus, minlength=modulus)


SLABS = tuple(range(3, 61, 3))           # first voxel layers of the two-voxel slabs below


def slab_residues(oracle, mask, cam, modulus, size=SIZE):
    """residues of the index of the first sample in `mask` INSIDE each two-voxel slab of the volume along z: the ball's
    background and its inside put a first sample of almost any property at index 0 or at the ball's surface, a slab moves it to
    every depth.  The sum over the slabs: rays (of some slab) whose sample at that position has the property"""
    n = S.geometric_counts(oracle, np.zeros(DIMS[::-1], dtype=np.uint8), size, cam)
    total = np.zeros(modulus, dtype=np.int64)
    for z0 in SLABS:
        slab = np.zeros(DIMS[::-1], dtype=bool)
        slab[z0:z0 + 2] = True
        total += residues(first_index(oracle, mask & slab, cam, size, n), modulus)
    return total


def empty_workgroups(n, threads):
    """workgroups of `threads` lanes none of whose rays has a sample: 512 = a 32 x 16 tile, 256 = its upper or lower 32 x 8"""
    h, w = n.shape
    th = S.TILE_H * threads // 512
    gy, gx = (h + S.TILE_H - 1) // S.TILE_H * (S.TILE_H // th), (w + S.TILE_W - 1) // S.TILE_W
    p = np.zeros((gy * th, gx * S.TILE_W), dtype=np.int64)
    p[:h, :w] = n
    per = p.reshape(gy, th, gx, S.TILE_W).max(axis=(1, 3))
    return int(np.count_nonzero(per == 0)), int(np.count_nonzero(per > 0))
