"""TEST INFRASTRUCTURE ONLY -- ctypes binding of tests/smooth_ref/smooth_ref.c, the CPU definition of vr_smooth_volume.

build(dir) compiles it with gcc (-O2 -std=c99 -ffp-contract=off -fno-fast-math) into `dir`.  The weights are inputs: pass one
array per axis as vr_smooth_weights wrote it (renderer.smooth_weights), or None for an axis whose sigma is 0.
"""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

SRC = Path(__file__).resolve().parent / "smooth_ref.c"
_FP = C.POINTER(C.c_float)


def build(out_dir) -> C.CDLL:
    so = Path(out_dir) / "libsmooth_ref.so"
    cmd = ["gcc", "-O2", "-std=c99", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", str(SRC), "-o", str(so), "-lm"]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        raise RuntimeError("building smooth_ref.c failed:\n" + proc.stdout + proc.stderr)
    lib = C.CDLL(str(so))
    common = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, _FP, C.c_int, _FP, C.c_int, _FP, C.c_int]
    lib.smooth_volume.restype = C.c_int
    lib.smooth_volume.argtypes = common + [C.c_void_p]
    lib.smooth_points.restype = C.c_int
    lib.smooth_points.argtypes = common + [C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_uint32)]
    return lib


def _weight_args(weights):
    """(keep-alive list, [wx, rx, wy, ry, wz, rz])"""
    keep, args = [], []
    assert len(weights) == 3
    for w in weights:
        if w is None:
            args += [None, -1]
        else:
            a = np.ascontiguousarray(w, dtype=np.float32)
            assert a.ndim == 1 and a.size % 2 == 1
            keep.append(a)
            args += [a.ctypes.data_as(_FP), (a.size - 1) // 2]
    return keep, args


def smooth(lib, volume: np.ndarray, weights) -> np.ndarray:
    """volume [z, y, x] uint8 / uint16; weights = (wx, wy, wz), None = no pass along that axis.  Returns the smoothed volume."""
    v = np.ascontiguousarray(volume)
    assert v.ndim == 3 and v.dtype in (np.uint8, np.uint16)
    nz, ny, nx = v.shape
    keep, wargs = _weight_args(weights)
    out = np.empty_like(v)
    rc = lib.smooth_volume(v.ctypes.data, v.dtype.itemsize, nx, ny, nz, *wargs, out.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"smooth_volume failed: {rc}")
    return out


def smooth_points(lib, volume: np.ndarray, weights, ijk) -> np.ndarray:
    """the smoothed value of the voxels ijk[n, 3] = (x, y, z), each from its own neighbourhood of `volume`"""
    v = np.ascontiguousarray(volume)
    assert v.ndim == 3 and v.dtype in (np.uint8, np.uint16)
    nz, ny, nx = v.shape
    keep, wargs = _weight_args(weights)
    p = np.ascontiguousarray(ijk, dtype=np.int32).reshape(-1, 3)
    out = np.zeros(p.shape[0], dtype=np.uint32)
    rc = lib.smooth_points(v.ctypes.data, v.dtype.itemsize, nx, ny, nz, *wargs, p.shape[0], p.ctypes.data_as(C.POINTER(C.c_int32)),
                           out.ctypes.data_as(C.POINTER(C.c_uint32)))
    if rc != 0:
        raise RuntimeError(f"smooth_points failed: {rc}")
    return out.astype(v.dtype)
