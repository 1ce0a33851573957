"""TEST INFRASTRUCTURE ONLY -- ctypes binding of tests/simplify_ref/simplify_ref.c, the CPU definition of vr_simplify_mesh.

build(dir) compiles it with gcc (-O2 -std=c99 -ffp-contract=off -fno-fast-math) into `dir`.
"""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

SRC = Path(__file__).resolve().parent / "simplify_ref.c"
_FP = C.POINTER(C.c_float)
_UP = C.POINTER(C.c_uint32)
_QP = C.POINTER(C.c_uint64)

OK, BAD_CELL, OVERFLOW, NO_MEMORY, BAD_INDEX = 0, 1, 2, 3, 4


class SimplifyError(RuntimeError):
    def __init__(self, code):
        super().__init__(f"simplify_mesh failed: {code}")
        self.code = code


def build(out_dir) -> C.CDLL:
    so = Path(out_dir) / "libsimplify_ref.so"
    cmd = ["gcc", "-O2", "-std=c99", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", str(SRC), "-o", str(so), "-lm"]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        raise RuntimeError("building simplify_ref.c failed:\n" + proc.stdout + proc.stderr)
    lib = C.CDLL(str(so))
    lib.simplify_mesh.restype = C.c_int
    lib.simplify_mesh.argtypes = [_FP, _FP, _UP, C.c_uint64, C.c_uint64, C.c_float, _FP, _FP, _UP, _QP, _QP, _UP]
    return lib


def simplify(lib, mesh, cell):
    """mesh = (positions [nv, 3] float32, normals [nv, 3] float32, triangles [nt, 3] uint32).  Returns the simplified mesh in the
    same form and rows [nv'] uint32, the input index of every output vertex.  SimplifyError(code) where the definition refuses."""
    pos, nrm, tri = (np.ascontiguousarray(a) for a in mesh)
    assert pos.dtype == np.float32 and nrm.dtype == np.float32 and tri.dtype == np.uint32
    assert pos.ndim == 2 and pos.shape[1] == 3 and nrm.shape == pos.shape and tri.ndim == 2 and tri.shape[1] == 3
    nv, nt = pos.shape[0], tri.shape[0]
    opos, onrm = np.zeros((nv, 3), dtype=np.float32), np.zeros((nv, 3), dtype=np.float32)
    otri, rows = np.zeros((nt, 3), dtype=np.uint32), np.zeros(nv, dtype=np.uint32)
    onv, ont = C.c_uint64(0), C.c_uint64(0)
    rc = lib.simplify_mesh(pos.ctypes.data_as(_FP), nrm.ctypes.data_as(_FP), tri.ctypes.data_as(_UP), nv, nt, float(cell),
                           opos.ctypes.data_as(_FP), onrm.ctypes.data_as(_FP), otri.ctypes.data_as(_UP), C.byref(onv), C.byref(ont),
                           rows.ctypes.data_as(_UP))
    if rc != OK:
        raise SimplifyError(rc)
    return (opos[:onv.value].copy(), onrm[:onv.value].copy(), otri[:ont.value].copy()), rows[:onv.value].copy()
