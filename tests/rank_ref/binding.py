"""TEST INFRASTRUCTURE ONLY -- ctypes binding of tests/rank_ref/rank_ref.c, the brute-force CPU definition of
vr_rank_filter_volume.  build(dir) compiles it with gcc (-O2 -std=c99) into `dir`."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

SRC = Path(__file__).resolve().parent / "rank_ref.c"
OFF, ERODE, DILATE, OPEN, CLOSE, MEDIAN = range(6)


def build(out_dir) -> C.CDLL:
    so = Path(out_dir) / "librank_ref.so"
    cmd = ["gcc", "-O2", "-std=c99", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", str(SRC), "-o", str(so)]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        raise RuntimeError("building rank_ref.c failed:\n" + proc.stdout + proc.stderr)
    lib = C.CDLL(str(so))
    lib.rank_volume.restype = C.c_int
    lib.rank_volume.argtypes = [C.c_void_p] + [C.c_int] * 8 + [C.c_void_p]
    lib.rank_points.restype = C.c_int
    lib.rank_points.argtypes = [C.c_void_p] + [C.c_int] * 9 + [C.POINTER(C.c_int32), C.POINTER(C.c_uint32)]
    return lib


def _radii(radius):
    r = np.broadcast_to(np.asarray(radius, dtype=np.int64), (3,))
    return int(r[0]), int(r[1]), int(r[2])


def rank(lib, volume: np.ndarray, op: int, radius) -> np.ndarray:
    """volume [z, y, x] uint8 / uint16; radius: a number or (rx, ry, rz).  Returns the filtered volume."""
    v = np.ascontiguousarray(volume)
    assert v.ndim == 3 and v.dtype in (np.uint8, np.uint16)
    nz, ny, nx = v.shape
    out = np.empty_like(v)
    rc = lib.rank_volume(v.ctypes.data, v.dtype.itemsize, nx, ny, nz, int(op), *_radii(radius), out.ctypes.data)
    if rc != 0:
        raise ValueError(f"rank_volume refused: {rc}")
    return out


def rank_points(lib, volume: np.ndarray, op: int, radius, ijk) -> np.ndarray:
    """ERODE, DILATE or MEDIAN at the voxels ijk[n, 3] = (x, y, z) of a linear [z, y, x] volume of any size"""
    v = volume
    assert v.ndim == 3 and v.dtype in (np.uint8, np.uint16) and v.flags.c_contiguous
    nz, ny, nx = v.shape
    p = np.ascontiguousarray(ijk, dtype=np.int32).reshape(-1, 3)
    out = np.zeros(p.shape[0], dtype=np.uint32)
    rc = lib.rank_points(v.ctypes.data, v.dtype.itemsize, nx, ny, nz, int(op), *_radii(radius), p.shape[0],
                         p.ctypes.data_as(C.POINTER(C.c_int32)), out.ctypes.data_as(C.POINTER(C.c_uint32)))
    if rc != 0:
        raise ValueError(f"rank_points refused: {rc}")
    return out.astype(v.dtype)
