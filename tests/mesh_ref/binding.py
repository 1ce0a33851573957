"""TEST INFRASTRUCTURE ONLY -- ctypes binding of tests/mesh_ref/mesh_ref.c, the CPU definition of vr_extract_isosurface.

build(dir) compiles it with gcc (-O2 -std=c99 -ffp-contract=off -fno-fast-math) into `dir`.
"""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

SRC = Path(__file__).resolve().parent / "mesh_ref.c"
_FP = C.POINTER(C.c_float)
_IP = C.POINTER(C.c_int)
_UP = C.POINTER(C.c_uint32)
_QP = C.POINTER(C.c_uint64)


def build(out_dir) -> C.CDLL:
    so = Path(out_dir) / "libmesh_ref.so"
    cmd = ["gcc", "-O2", "-std=c99", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", str(SRC), "-o", str(so), "-lm"]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        raise RuntimeError("building mesh_ref.c failed:\n" + proc.stdout + proc.stderr)
    lib = C.CDLL(str(so))
    lib.mesh_extract.restype = C.c_int
    lib.mesh_extract.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, _FP, _IP, _IP, _FP, _FP, _UP,
                                 C.c_uint64, C.c_uint64, _QP, _QP]
    lib.mesh_case_swapped.restype = C.c_int
    lib.mesh_case_swapped.argtypes = [C.c_int]
    return lib


def iso_stored(iso, dtype, u16_offset=True) -> float:
    """step 2: iso_s = float(iso + 1000) for 16-bit data under VR_QUIRK_U16_OFFSET, float(iso) otherwise"""
    return float(np.float32(int(iso) + (1000 if np.dtype(dtype).itemsize == 2 and u16_offset else 0)))


def extract(lib, volume: np.ndarray, iso_s, spacing=(1.0, 1.0, 1.0), box=None):
    """volume [z, y, x] uint8 / uint16, iso_s in stored units, spacing (x, y, z); box = ((i0, j0, k0), (i1, j1, k1)): only the
    cells i0 <= i < i1, ... (see mesh_ref.c).  Returns positions [nv, 3], normals [nv, 3] float32 and triangles [nt, 3] uint32."""
    v = volume if volume.flags["C_CONTIGUOUS"] else np.ascontiguousarray(volume)
    assert v.ndim == 3 and v.dtype in (np.uint8, np.uint16)
    nz, ny, nx = v.shape
    sp = np.asarray(spacing, dtype=np.float32)
    assert sp.shape == (3,)
    c0 = c1 = None
    if box is not None:
        lo, hi = np.asarray(box[0], dtype=np.intc), np.asarray(box[1], dtype=np.intc)
        c0, c1 = lo.ctypes.data_as(_IP), hi.ctypes.data_as(_IP)
    nv, nt = C.c_uint64(0), C.c_uint64(0)
    head = (v.ctypes.data, v.dtype.itemsize, nx, ny, nz, float(iso_s), sp.ctypes.data_as(_FP), c0, c1)
    rc = lib.mesh_extract(*head, None, None, None, 0, 0, C.byref(nv), C.byref(nt))
    if rc != 0:
        raise RuntimeError(f"mesh_extract (count) failed: {rc}")
    pos = np.zeros((nv.value, 3), dtype=np.float32)
    nrm = np.zeros((nv.value, 3), dtype=np.float32)
    tri = np.zeros((nt.value, 3), dtype=np.uint32)
    rc = lib.mesh_extract(*head, pos.ctypes.data_as(_FP), nrm.ctypes.data_as(_FP), tri.ctypes.data_as(_UP), nv.value, nt.value,
                          C.byref(nv), C.byref(nt))
    if rc != 0:
        raise RuntimeError(f"mesh_extract failed: {rc}")
    assert (nv.value, nt.value) == (pos.shape[0], tri.shape[0])
    return pos, nrm, tri
