"""TEST INFRASTRUCTURE ONLY -- ctypes binding of tests/shade_ref/shade_ref.c, the CPU definition of gradient-lit compositing.

build(dir) compiles it with gcc (-O2 -std=c99 -ffp-contract=off -fno-fast-math) into `dir`; render() takes the inputs of
oracle.OracleParams plus the shading coefficients and returns RGBA and per-pixel sample counts.
"""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

SRC = Path(__file__).resolve().parent / "shade_ref.c"


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
        ("alpha_scale", C.c_float),
        ("ambient", C.c_float), ("diffuse", C.c_float), ("specular", C.c_float),
        ("shininess", C.c_int32),
    ]


def build(out_dir) -> C.CDLL:
    so = Path(out_dir) / "libshade_ref.so"
    cmd = ["gcc", "-O2", "-std=c99", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", str(SRC), "-o", str(so), "-lm"]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        raise RuntimeError("building shade_ref.c failed:\n" + proc.stdout + proc.stderr)
    lib = C.CDLL(str(so))
    lib.shade_render.restype = C.c_int
    lib.shade_render.argtypes = [C.POINTER(_Params), C.POINTER(C.c_float), C.POINTER(C.c_uint32)]
    return lib


def render(lib, volume: np.ndarray, p, ambient=0.15, diffuse=0.65, specular=0.2, shininess=16):
    """volume [z, y, x]; p = oracle.OracleParams (is_mip is ignored: the mode is an option of the composite mode).
    Returns (rgba[h, w, 4], spp[h, w]); rows outside [row_begin, row_end) are zero."""
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
    q.alpha_scale = p.alpha_scale
    q.ambient, q.diffuse, q.specular, q.shininess = float(ambient), float(diffuse), float(specular), int(shininess)
    rgba = np.zeros((p.img_h, p.img_w, 4), dtype=np.float32)
    spp = np.zeros((p.img_h, p.img_w), dtype=np.uint32)
    rc = lib.shade_render(C.byref(q), rgba.ctypes.data_as(C.POINTER(C.c_float)), spp.ctypes.data_as(C.POINTER(C.c_uint32)))
    if rc != 0:
        raise RuntimeError(f"shade_render failed: {rc}")
    return rgba, spp
