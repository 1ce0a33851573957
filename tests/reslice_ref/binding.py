"""TEST INFRASTRUCTURE ONLY -- ctypes binding of tests/reslice_ref/reslice_ref.c, the CPU definition of the reslice mode.

build(dir) compiles it with gcc (-O2 -std=c99 -ffp-contract=off -fno-fast-math) into `dir`; render() takes a volume, the 12
geometry floats and the mode's settings and returns RGBA, the read-back values and the per-pixel sample counts.
"""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

SRC = Path(__file__).resolve().parent / "reslice_ref.c"
MODES = {"mip": 0, "minip": 1, "mean": 2}


class _Params(C.Structure):
    _fields_ = [
        ("img_w", C.c_int32), ("img_h", C.c_int32), ("row_begin", C.c_int32), ("row_end", C.c_int32), ("trunc_grid", C.c_int32),
        ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("bytes_per_voxel", C.c_int32),
        ("volume", C.c_void_p),
        ("geom", C.c_float * 12),
        ("mode", C.c_int32), ("n", C.c_int32), ("filter", C.c_int32),
        ("min_val", C.c_int32), ("max_val", C.c_int32),
        ("tf_rgba", C.POINTER(C.c_float)), ("tf_len", C.c_int32),
        ("u16_offset", C.c_int32),
    ]


def build(out_dir) -> C.CDLL:
    so = Path(out_dir) / "libreslice_ref.so"
    cmd = ["gcc", "-O2", "-std=c99", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", str(SRC), "-o", str(so), "-lm"]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        raise RuntimeError("building reslice_ref.c failed:\n" + proc.stdout + proc.stderr)
    lib = C.CDLL(str(so))
    lib.reslice_render.restype = C.c_int
    lib.reslice_render.argtypes = [C.POINTER(_Params), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint32)]
    return lib


def render(lib, volume: np.ndarray, geom, img_w: int, img_h: int, mode="mip", n=1, filt=0, min_val=0, max_val=255,
           tf_rgba=None, u16_offset=True, row_begin=0, row_end=-1, trunc_grid=False):
    """volume [z, y, x]; geom = the 12 floats of vr_set_reslice; min_val / max_val = the window as the kernel sees it (the
    +1000 of the u16 offset included).  Returns (rgba[h, w, 4], values[h, w], cnt[h, w]); rows outside [row_begin, row_end)
    are zero (values NaN)."""
    v = np.ascontiguousarray(volume)
    assert v.ndim == 3 and v.dtype in (np.uint8, np.uint16)
    nz, ny, nx = v.shape
    q = _Params()
    q.img_w, q.img_h = img_w, img_h
    q.row_begin = row_begin
    q.row_end = img_h if row_end < 0 else row_end
    q.trunc_grid = 1 if trunc_grid else 0
    q.nx, q.ny, q.nz = nx, ny, nz
    q.bytes_per_voxel = v.dtype.itemsize
    q.volume = v.ctypes.data
    g = np.ascontiguousarray(geom, dtype=np.float32).reshape(12)
    for i in range(12):
        q.geom[i] = float(g[i])
    q.mode = MODES[mode] if isinstance(mode, str) else int(mode)
    q.n, q.filter = int(n), int(filt)
    q.min_val, q.max_val = int(min_val), int(max_val)
    tf = None
    if tf_rgba is not None:
        tf = np.ascontiguousarray(tf_rgba, dtype=np.float32).reshape(-1, 4)
        q.tf_rgba = tf.ctypes.data_as(C.POINTER(C.c_float))
        q.tf_len = tf.shape[0]
    q.u16_offset = 1 if u16_offset else 0
    rgba = np.zeros((img_h, img_w, 4), dtype=np.float32)
    values = np.full((img_h, img_w), np.nan, dtype=np.float32)
    cnt = np.zeros((img_h, img_w), dtype=np.uint32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    rc = lib.reslice_render(C.byref(q), fp(rgba), fp(values), cnt.ctypes.data_as(C.POINTER(C.c_uint32)))
    if rc != 0:
        raise RuntimeError(f"reslice_render failed: {rc}")
    return rgba, values, cnt
