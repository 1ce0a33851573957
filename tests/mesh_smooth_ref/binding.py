"""TEST INFRASTRUCTURE ONLY -- ctypes binding of tests/mesh_smooth_ref/mesh_smooth_ref.c, the CPU definition of vr_smooth_mesh.

build(dir) compiles it with gcc (-O2 -std=c99 -ffp-contract=off -fno-fast-math) into `dir`.
"""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

SRC = Path(__file__).resolve().parent / "mesh_smooth_ref.c"
_FP = C.POINTER(C.c_float)
_UP = C.POINTER(C.c_uint32)
_BP = C.POINTER(C.c_uint8)
_QP = C.POINTER(C.c_uint64)

OK, BAD_PARAMETER, TOO_MANY_PAIRS, NO_MEMORY, BAD_INDEX = 0, 1, 2, 3, 4


class SmoothError(RuntimeError):
    def __init__(self, code):
        super().__init__(f"mesh_smooth failed: {code}")
        self.code = code


def build(out_dir) -> C.CDLL:
    so = Path(out_dir) / "libmesh_smooth_ref.so"
    cmd = ["gcc", "-O2", "-std=c99", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", str(SRC), "-o", str(so), "-lm"]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        raise RuntimeError("building mesh_smooth_ref.c failed:\n" + proc.stdout + proc.stderr)
    lib = C.CDLL(str(so))
    lib.mesh_smooth.restype = C.c_int
    lib.mesh_smooth.argtypes = [_FP, _UP, C.c_uint64, C.c_uint64, C.c_int, C.c_float, C.c_float, C.c_int, _FP, _FP, _BP, _QP]
    return lib


def smooth(lib, mesh, iterations=10, lam=0.5, mu=-0.53, fix_boundary=True):
    """mesh = (positions [nv, 3] float32, normals [nv, 3] float32, triangles [nt, 3] uint32).  Returns the smoothed mesh in the
    same form (the triangles are the input's array) and fixed [nv] bool.  iterations == 0 returns the input, normals included, as
    vr_smooth_mesh's step 7 does.  SmoothError(code) where the definition refuses."""
    pos, nrm, tri = (np.ascontiguousarray(a) for a in mesh)
    assert pos.dtype == np.float32 and nrm.dtype == np.float32 and tri.dtype == np.uint32
    assert pos.ndim == 2 and pos.shape[1] == 3 and nrm.shape == pos.shape and tri.ndim == 2 and tri.shape[1] == 3
    nv, nt = pos.shape[0], tri.shape[0]
    opos, onrm = np.zeros((nv, 3), dtype=np.float32), np.zeros((nv, 3), dtype=np.float32)
    fixed, n_fixed = np.zeros(nv, dtype=np.uint8), C.c_uint64(0)
    rc = lib.mesh_smooth(pos.ctypes.data_as(_FP), tri.ctypes.data_as(_UP), nv, nt, int(iterations), float(lam), float(mu), 1 if fix_boundary else 0,
                         opos.ctypes.data_as(_FP), onrm.ctypes.data_as(_FP), fixed.ctypes.data_as(_BP), C.byref(n_fixed))
    if rc != OK:
        raise SmoothError(rc)
    assert n_fixed.value == int(fixed.sum())
    if iterations == 0:
        return (pos.copy(), nrm.copy(), tri), np.zeros(nv, dtype=bool)
    return (opos, onrm, tri), fixed.astype(bool)
