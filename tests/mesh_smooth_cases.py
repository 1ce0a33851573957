"""TEST INFRASTRUCTURE ONLY -- shared by tests/test_mesh_smooth_cpu.py and tests/test_mesh_smooth_gpu.py: an independent numpy
statement of vr_smooth_mesh's definition (include/vr_core.h, steps 2 to 6), the consequences of its step 8 as checks on any (input,
output) pair, and the volumes whose meshes both files smooth.  Nothing here knows how a smoothing was computed."""
from __future__ import annotations

import importlib.util
from pathlib import Path

import numpy as np

_spec = importlib.util.spec_from_file_location("simplify_cases", Path(__file__).resolve().parent / "simplify_cases.py")
_S = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_S)
random_volume, ties_volume, ball_volume = _S.random_volume, _S.ties_volume, _S.ball_volume

SPACING = (0.5, 1.0, 2.0)
DEFAULTS = dict(iterations=10, lam=0.5, mu=-0.53, fix_boundary=True)
CUT_X = 40


def cut_ball_volume():
    """the ball's first CUT_X columns: the surface is open where it meets the plane x = CUT_X - 1"""
    return np.ascontiguousarray(ball_volume()[:, :, :CUT_X])


# ---------------------------------------------------------------- the definition
def graph(nv: int, tri: np.ndarray):
    """step 2: (start [nv + 1], neighbours, multiplicity): row i of the compressed rows holds N(i) in ascending order and, beside
    every neighbour, the number of pairs (i, j)"""
    t = tri.astype(np.int64)
    a = np.concatenate([t[:, 0], t[:, 1], t[:, 1], t[:, 2], t[:, 2], t[:, 0]])
    b = np.concatenate([t[:, 1], t[:, 0], t[:, 2], t[:, 1], t[:, 0], t[:, 2]])
    keep = a != b
    keys, mult = np.unique(a[keep] << 32 | b[keep], return_counts=True)
    start = np.zeros(nv + 1, dtype=np.int64)
    np.cumsum(np.bincount(keys >> 32, minlength=nv), out=start[1:])
    return start, keys & 0xFFFFFFFF, mult


def fixed_vertices(nv: int, tri: np.ndarray, fix_boundary) -> np.ndarray:
    """step 3: [nv] bool"""
    start, nbr, mult = graph(nv, tri)
    fixed = np.zeros(nv, dtype=bool)
    if fix_boundary:
        owner = np.repeat(np.arange(nv), np.diff(start))
        fixed[owner[mult == 1]] = True
        fixed[nbr[mult == 1]] = True
    return fixed


def ranked_sum(values: np.ndarray, start: np.ndarray, source: np.ndarray) -> np.ndarray:
    """per row i: ((0 + values[source[start[i]]]) + values[source[start[i] + 1]]) + ... in float32, one rank of every row at a
    time, so that each row's additions happen in the row's order"""
    n = start.size - 1
    count = np.diff(start)
    acc = np.zeros((n, values.shape[1]), dtype=np.float32)
    for rank in range(int(count.max()) if n else 0):
        rows = np.flatnonzero(count > rank)
        acc[rows] = acc[rows] + values[source[start[rows] + rank]]
    assert acc.dtype == np.float32
    return acc


def numpy_step(p: np.ndarray, start, nbr, moves, phi) -> np.ndarray:
    """step 4"""
    k = np.diff(start)
    acc = ranked_sum(p, start, nbr)
    out = p.copy()
    m = acc[moves] / k[moves].astype(np.float32)[:, None]
    d = m - p[moves]
    s = np.float32(phi) * d
    out[moves] = p[moves] + s
    assert m.dtype == d.dtype == s.dtype == out.dtype == np.float32
    return out


def numpy_normals(p: np.ndarray, tri: np.ndarray) -> np.ndarray:
    """step 6"""
    nv = p.shape[0]
    t = tri.astype(np.int64)
    u, w = p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]]
    face = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], axis=1)
    assert face.dtype == np.float32
    flat = t.ravel()
    order = np.argsort(flat, kind="stable")                  # by vertex; within a vertex ascending (t, corner)
    start = np.zeros(nv + 1, dtype=np.int64)
    np.cumsum(np.bincount(flat, minlength=nv), out=start[1:])
    s = ranked_sum(face, start, order // 3)
    dot = (s[:, 2] * s[:, 2] + s[:, 1] * s[:, 1]) + s[:, 0] * s[:, 0]
    n = np.zeros_like(s)
    some = dot != 0
    rn = np.float32(1.0) / np.sqrt(dot[some])
    n[some] = s[some] * rn[:, None]
    assert dot.dtype == rn.dtype == n.dtype == np.float32
    return n


def numpy_smooth(mesh, iterations=10, lam=0.5, mu=-0.53, fix_boundary=True):
    """steps 2 to 7: returns ((positions, normals, triangles), fixed)"""
    pos, nrm, tri = mesh
    nv = pos.shape[0]
    if iterations == 0:
        return (pos.copy(), nrm.copy(), tri), np.zeros(nv, dtype=bool)
    start, nbr, _ = graph(nv, tri)
    fixed = fixed_vertices(nv, tri, fix_boundary)
    moves = np.flatnonzero(~fixed & (np.diff(start) > 0))
    p = pos.astype(np.float32).copy()
    with np.errstate(all="ignore"):
        for _ in range(iterations):
            p = numpy_step(p, start, nbr, moves, lam)
            if mu != 0:
                p = numpy_step(p, start, nbr, moves, mu)
        return (p, numpy_normals(p, tri), tri), fixed


# ---------------------------------------------------------------- step 8
def consequences(source, result, fixed) -> str:
    """'' when `result` has what step 8 promises of a smoothing of `source` with the fixed vertices `fixed`; else what is wrong"""
    (spos, _, stri), (pos, nrm, tri) = source, result
    if pos.shape != spos.shape or nrm.shape != spos.shape:
        return "V changed"
    if tri.shape != stri.shape or not np.array_equal(tri, stri):
        return "the triangles changed"
    if not np.array_equal(pos[fixed].view(np.uint32), spos[fixed].view(np.uint32)):
        return "a fixed vertex moved"
    unreferenced = np.ones(pos.shape[0], dtype=bool)
    unreferenced[tri.ravel()] = False
    if not np.array_equal(pos[unreferenced].view(np.uint32), spos[unreferenced].view(np.uint32)):
        return "a vertex without a neighbour moved"
    if np.any(nrm[unreferenced].view(np.uint32) != 0):
        return "a vertex without a triangle has a normal"
    length = np.sqrt((nrm.astype(np.float64) ** 2).sum(axis=1))
    if np.any((np.abs(length - 1.0) > 1e-5) & (length != 0.0)):
        return "a normal is neither of unit length nor zero"
    return ""


def degree_and_multiplicity(nv: int, tri: np.ndarray):
    """(the largest k_i, the largest edge multiplicity)"""
    start, _, mult = graph(nv, tri)
    return int(np.diff(start).max()), int(mult.max())
