"""TEST INFRASTRUCTURE ONLY -- ctypes binding of tests/iso_ref/iso_ref.c, the CPU definition of the isosurface mode.

build(dir) compiles it with gcc (-O2 -std=c99 -ffp-contract=off -fno-fast-math) into `dir`; render() takes the inputs of
oracle.OracleParams plus the iso value and returns RGBA, depth, per-pixel sample counts and, on request, the shading normal.
"""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

SRC = Path(__file__).resolve().parent / "iso_ref.c"


class _Params(C.Structure):
    _fields_ = [
        ("img_w", C.c_int32), ("img_h", C.c_int32), ("row_begin", C.c_int32), ("row_end", C.c_int32), ("trunc_grid", C.c_int32),
        ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("bytes_per_voxel", C.c_int32),
        ("volume", C.c_void_p),
        ("cam", C.c_float * 21),
        ("voxel_size", C.c_float * 3),
        ("min_val", C.c_int32), ("max_val", C.c_int32),
        ("view_top", C.c_int32), ("view_bottom", C.c_int32), ("filter", C.c_int32), ("accum", C.c_int32), ("max_steps", C.c_int32),
        ("tf_rgba", C.POINTER(C.c_float)), ("tf_len", C.c_int32),
        ("iso_value", C.c_int32), ("u16_offset", C.c_int32),
    ]


def build(out_dir) -> C.CDLL:
    so = Path(out_dir) / "libiso_ref.so"
    cmd = ["gcc", "-O2", "-std=c99", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", str(SRC), "-o", str(so), "-lm"]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        raise RuntimeError("building iso_ref.c failed:\n" + proc.stdout + proc.stderr)
    lib = C.CDLL(str(so))
    lib.iso_render.restype = C.c_int
    lib.iso_render.argtypes = [C.POINTER(_Params), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_float)]
    return lib


def render(lib, volume: np.ndarray, p, iso: int, u16_offset: bool = True, want_normal: bool = False):
    """volume [z, y, x]; p = oracle.OracleParams (is_mip / alpha_scale are ignored: the mode ignores them).
    Returns (rgba[h, w, 4], depth[h, w], spp[h, w]) or, with want_normal, (..., normal[h, w, 3]); rows outside
    [row_begin, row_end) are zero (depth +inf)."""
    v = np.ascontiguousarray(volume)
    assert v.ndim == 3 and v.dtype in (np.uint8, np.uint16)
    nz, ny, nx = v.shape
    q = _Params()
    q.img_w, q.img_h = p.img_w, p.img_h
    q.row_begin = p.row_begin
    q.row_end = p.img_h if p.row_end < 0 else p.row_end
    q.trunc_grid = p.trunc_grid
    q.nx, q.ny, q.nz = nx, ny, nz
    q.bytes_per_voxel = v.dtype.itemsize
    q.volume = v.ctypes.data
    cam = np.ascontiguousarray(p.cam, dtype=np.float32)
    for i in range(21):
        q.cam[i] = float(cam[i])
    for i in range(3):
        q.voxel_size[i] = p.voxel_size[i]
    q.min_val, q.max_val = p.min_val, p.max_val
    q.view_top, q.view_bottom, q.filter, q.accum, q.max_steps = p.view_top, p.view_bottom, p.filter, p.accum, p.max_steps
    tf = None
    if p.tf_rgba is not None:
        tf = np.ascontiguousarray(p.tf_rgba, dtype=np.float32).reshape(-1, 4)
        q.tf_rgba = tf.ctypes.data_as(C.POINTER(C.c_float))
        q.tf_len = tf.shape[0]
    q.iso_value = int(iso)
    q.u16_offset = 1 if u16_offset else 0
    rgba = np.zeros((p.img_h, p.img_w, 4), dtype=np.float32)
    depth = np.full((p.img_h, p.img_w), np.inf, dtype=np.float32)
    spp = np.zeros((p.img_h, p.img_w), dtype=np.uint32)
    normal = np.zeros((p.img_h, p.img_w, 3), dtype=np.float32) if want_normal else None
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    rc = lib.iso_render(C.byref(q), fp(rgba), fp(depth), spp.ctypes.data_as(C.POINTER(C.c_uint32)),
                        fp(normal) if want_normal else None)
    if rc != 0:
        raise RuntimeError(f"iso_render failed: {rc}")
    return (rgba, depth, spp, normal) if want_normal else (rgba, depth, spp)

