"""TEST INFRASTRUCTURE ONLY -- the 12-bit packed format of the ray-ordered sample stream (csrc/vr_stream_pack.h, vr_stream.hip),
for tests/test_ray_stream_pack_cpu.py and tests/test_ray_stream_pack_gpu.py.  Geometry, cameras, modes and the unpacked size
model are tests/ray_stream_cases.py's (S below); here is what the packed format adds: groups of 8, the size model, volumes whose
bits and base matter, and constant volumes that end every ray at each position of a group of 8.

Volumes are indexed [z, y, x]; sizes are (width, height).
"""
import importlib.util
from pathlib import Path

import numpy as np

_spec = importlib.util.spec_from_file_location("ray_stream_cases", Path(__file__).resolve().parent / "ray_stream_cases.py")
S = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(S)

STREAM12 = "raymarch_stream12_kernel"
G12 = 8                                 # kStreamGroup12: samples a lane reads with one 12-byte load
SPAN12 = 4095                           # kStreamSpan12
PACK_MIN_RAW_BYTES = 256 << 20          # kStreamPackMinRawBytes: the automatic mode packs above it
DIMS = S.RESIDUE_DIMS
SIZE = S.RESIDUE_SIZE


def packed_block_groups(n_local):
    """ceil(max n / 8) of every stream block"""
    return (S.block_groups(n_local) * S.G + G12 - 1) // G12      # ceil_8(ceil_4(n)) == ceil_8(n)


def packed_stream_bytes(n_local):
    """what VolumeCopies::ensureRayStream allocates for a packed stream: 12 bytes per lane per group of 8 (768 per group), 16
    bytes of slack, a 16-bit count per lane, a 64-bit offset per block and one more"""
    groups = packed_block_groups(n_local)
    blocks = groups.size
    return int(groups.sum()) * 768 + 16 + blocks * 64 * 2 + (blocks + 1) * 8


def raw_sample_bytes(n_local, bytes_per_voxel=2):
    """the samples alone of the unpacked stream: what the automatic mode compares with PACK_MIN_RAW_BYTES"""
    return int(S.block_groups(n_local).sum()) * 64 * S.G * bytes_per_voxel


# ---------------------------------------------------------------------------------------------------------------
# rays that end at each position of a group of 8 by the 0.95 test
# ---------------------------------------------------------------------------------------------------------------
# A constant volume of value 204 under the window (0, 255): s = 0.8, a = 0.8 * alpha per sample, dest.a = 1 - (1 - a)^k.  A ray
# composites `count` samples when (1 - a)^(count - 1) > 0.05 >= (1 - a)^count (tests/ray_stream_cases.py: CONSTANT_CASES, 11 and
# 12).  alpha puts 0.05 in the middle: 1 - a = 0.05^(1 / (count - 0.5)), so (1 - a)^count and (1 - a)^(count - 1) are 0.05 times
# and divided by (1 - a)^0.5 -- 0.82 .. 0.90 for the counts here, thousands of fp32 roundings away.  Rounded to four decimals.
END_VALUE = 204
END_COUNTS = tuple(range(8, 16))        # 8 k + r for k = 1, r = 0 .. 7


def end_alpha(count):
    return round((1.0 - 0.05 ** (1.0 / (count - 0.5))) / 0.8, 4)


END_CASES = [(END_VALUE, end_alpha(c), c) for c in END_COUNTS]


def constant_volume(value):
    return np.full(DIMS[::-1], value, dtype=np.uint16)


# ---------------------------------------------------------------------------------------------------------------
# volumes whose bits and whose base matter
# ---------------------------------------------------------------------------------------------------------------
def pattern_volume():
    """0x000 / 0xFFF / 0x555 / 0xAAA alternating along x, shifted by one per row and by two per slice: neighbouring samples of a
    ray and neighbouring fields of a group differ in every bit"""
    z, y, x = np.indices(DIMS[::-1])
    return np.array([0x000, 0xFFF, 0x555, 0xAAA], dtype=np.uint16)[(x + y + 2 * z) % 4]


OFFSET_BASE = 1000


def offset_volume(oracle):
    """the 12-bit noise ball with its extremes pinned to 0 and 4095, offset by 1000: range [1000, 5095], span 4095"""
    vol = oracle.gen_noise_ball(DIMS, 2, 0x5678).astype(np.uint16) & 0xFFF
    vol[0, 0, 0] = 0
    vol[0, 0, 1] = 4095
    return (vol + OFFSET_BASE).astype(np.uint16)


# windows over [1000, 5095]: containing it (the no-clamp instance), cutting into it from below, from above, and wholly below the
# base (every sample clamps to the window's top)
OFFSET_WINDOWS = [(900, 5200), (2000, 5200), (900, 3000), (100, 900)]


def span_4096_volume(oracle):
    """one value more than the format holds: [0, 4096]"""
    vol = oracle.gen_noise_ball(DIMS, 2, 0x5678).astype(np.uint16) & 0xFFF
    vol[0, 0, 0] = 0
    vol[0, 0, 1] = 4096
    return vol
