"""TEST INFRASTRUCTURE ONLY -- ctypes binding of tests/components_ref/components_ref.c, the CPU definition of
vr_label_components, vr_select_components and vr_extract_components.

build(dir) compiles it with gcc (-O2 -std=c99 -ffp-contract=off -fno-fast-math) into `dir`.
"""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

SRC = Path(__file__).resolve().parent / "components_ref.c"
_FP = C.POINTER(C.c_float)
_UP = C.POINTER(C.c_uint32)
_QP = C.POINTER(C.c_uint64)
_IP = C.POINTER(C.c_int32)
_BP = C.POINTER(C.c_uint8)


def build(out_dir) -> C.CDLL:
    so = Path(out_dir) / "libcomponents_ref.so"
    cmd = ["gcc", "-O2", "-std=c99", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", str(SRC), "-o", str(so), "-lm"]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        raise RuntimeError("building components_ref.c failed:\n" + proc.stdout + proc.stderr)
    lib = C.CDLL(str(so))
    lib.comp_label.restype = C.c_int64
    lib.comp_label.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, _UP]
    lib.comp_records.restype = C.c_int
    lib.comp_records.argtypes = [_UP, C.c_int, C.c_int, C.c_int, C.c_uint64, _QP, _QP, _IP]
    lib.comp_select.restype = C.c_int
    lib.comp_select.argtypes = [_QP, C.c_uint64, C.c_uint64, C.c_uint64, _BP]
    lib.comp_extract.restype = C.c_int
    lib.comp_extract.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, _FP, _UP, _BP, _FP, _FP, _UP,
                                 C.c_uint64, C.c_uint64, _QP, _QP]
    return lib


def iso_stored(iso, dtype, u16_offset=True) -> float:
    """step 1: iso_s = float(iso + 1000) for 16-bit data under VR_QUIRK_U16_OFFSET, float(iso) otherwise"""
    return float(np.float32(int(iso) + (1000 if np.dtype(dtype).itemsize == 2 and u16_offset else 0)))


def _volume(volume):
    v = volume if volume.flags["C_CONTIGUOUS"] else np.ascontiguousarray(volume)
    assert v.ndim == 3 and v.dtype in (np.uint8, np.uint16)
    return v


def label(lib, volume: np.ndarray, iso_s):
    """volume [z, y, x] uint8 / uint16, iso_s in stored units.  Returns (labels [z, y, x] uint32, records): records is a dict of
    voxels [n] uint64, first_voxel [n] uint64, bbox [n, 6] int32 and selected [n] bool (all True), entry label - 1."""
    v = _volume(volume)
    nz, ny, nx = v.shape
    labels = np.zeros(v.shape, dtype=np.uint32)
    n = lib.comp_label(v.ctypes.data, v.dtype.itemsize, nx, ny, nz, float(iso_s), labels.ctypes.data_as(_UP))
    if n < 0:
        raise RuntimeError(f"comp_label failed: {n}")
    voxels, first = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    bbox = np.zeros((n, 6), dtype=np.int32)
    rc = lib.comp_records(labels.ctypes.data_as(_UP), nx, ny, nz, n, voxels.ctypes.data_as(_QP), first.ctypes.data_as(_QP), bbox.ctypes.data_as(_IP))
    if rc != 0:
        raise RuntimeError(f"comp_records failed: {rc}")
    return labels, dict(voxels=voxels, first_voxel=first, bbox=bbox, selected=np.ones(n, dtype=bool))


def select(lib, voxels: np.ndarray, min_voxels=0, keep_largest=0) -> np.ndarray:
    """step 6's rule on the records' voxel counts -> selected [n] bool"""
    vx = np.ascontiguousarray(voxels, dtype=np.uint64)
    sel = np.zeros(vx.size, dtype=np.uint8)
    rc = lib.comp_select(vx.ctypes.data_as(_QP), vx.size, int(min_voxels), int(keep_largest), sel.ctypes.data_as(_BP))
    if rc != 0:
        raise RuntimeError(f"comp_select failed: {rc}")
    return sel.astype(bool)


def extract(lib, volume: np.ndarray, iso_s, labels: np.ndarray, selected: np.ndarray, spacing=(1.0, 1.0, 1.0)):
    """step 7: the mesh of the selected components.  Returns positions [nv, 3], normals [nv, 3] float32, triangles [nt, 3] uint32."""
    v = _volume(volume)
    nz, ny, nx = v.shape
    lab = np.ascontiguousarray(labels, dtype=np.uint32)
    assert lab.shape == v.shape
    sel = np.ascontiguousarray(selected, dtype=np.uint8)
    assert sel.size >= int(lab.max(initial=0))
    sp = np.asarray(spacing, dtype=np.float32)
    assert sp.shape == (3,)
    nv, nt = C.c_uint64(0), C.c_uint64(0)
    head = (v.ctypes.data, v.dtype.itemsize, nx, ny, nz, float(iso_s), sp.ctypes.data_as(_FP), lab.ctypes.data_as(_UP), sel.ctypes.data_as(_BP))
    rc = lib.comp_extract(*head, None, None, None, 0, 0, C.byref(nv), C.byref(nt))
    if rc != 0:
        raise RuntimeError(f"comp_extract (count) failed: {rc}")
    pos = np.zeros((nv.value, 3), dtype=np.float32)
    nrm = np.zeros((nv.value, 3), dtype=np.float32)
    tri = np.zeros((nt.value, 3), dtype=np.uint32)
    rc = lib.comp_extract(*head, pos.ctypes.data_as(_FP), nrm.ctypes.data_as(_FP), tri.ctypes.data_as(_UP), nv.value, nt.value,
                          C.byref(nv), C.byref(nt))
    if rc != 0:
        raise RuntimeError(f"comp_extract failed: {rc}")
    assert (nv.value, nt.value) == (pos.shape[0], tri.shape[0])
    return pos, nrm, tri
