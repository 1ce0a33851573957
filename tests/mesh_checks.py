"""TEST INFRASTRUCTURE ONLY -- properties of an indexed triangle mesh in numpy, shared by tests/test_mesh_cpu.py and
tests/test_mesh_gpu.py.  Nothing here knows how the mesh was made."""
from __future__ import annotations

import numpy as np


def directed_edges(tri: np.ndarray) -> np.ndarray:
    """every triangle's three directed edges as a << 32 | b"""
    t = tri.astype(np.uint64)
    return np.concatenate([t[:, 0] << np.uint64(32) | t[:, 1], t[:, 1] << np.uint64(32) | t[:, 2], t[:, 2] << np.uint64(32) | t[:, 0]])


def closed_and_oriented(tri: np.ndarray) -> str:
    """'' when every directed edge occurs exactly once and its reverse exactly once (a closed, consistently oriented, edge-manifold
    surface); else what is wrong"""
    e = directed_edges(tri)
    keys, counts = np.unique(e, return_counts=True)
    if np.any(counts != 1):
        return f"{int((counts != 1).sum())} directed edges occur more than once"
    rev = np.sort((keys & np.uint64(0xFFFFFFFF)) << np.uint64(32) | keys >> np.uint64(32))
    if not np.array_equal(rev, keys):
        return f"{int(np.setdiff1d(keys, rev).size)} directed edges have no reverse"
    return ""


def euler_characteristic(n_vertices: int, tri: np.ndarray) -> int:
    """V - E + F with E the undirected edges"""
    e = directed_edges(tri)
    lo, hi = np.minimum(e >> np.uint64(32), e & np.uint64(0xFFFFFFFF)), np.maximum(e >> np.uint64(32), e & np.uint64(0xFFFFFFFF))
    return int(n_vertices) - int(np.unique(lo << np.uint64(32) | hi).size) + int(tri.shape[0])


def every_vertex_referenced(n_vertices: int, tri: np.ndarray) -> bool:
    return np.array_equal(np.unique(tri), np.arange(n_vertices, dtype=tri.dtype))


def cross_products(pos: np.ndarray, tri: np.ndarray) -> np.ndarray:
    """(p1 - p0) x (p2 - p0) per triangle, float64"""
    p = pos.astype(np.float64)[tri.astype(np.int64)]
    return np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])


def signed_volume(pos: np.ndarray, tri: np.ndarray) -> float:
    """sum of p0 . (p1 x p2) / 6, float64: positive when the winding is outward"""
    p = pos.astype(np.float64)[tri.astype(np.int64)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


def same_bits(got, want) -> str:
    """'' when the two meshes (positions, normals, triangles) are equal as arrays, bit for bit"""
    for name, g, w in zip(("positions", "normals", "triangles"), got, want):
        if g.shape != w.shape:
            return f"{name}: shape {g.shape} against {w.shape}"
        gb, wb = np.ascontiguousarray(g).view(np.uint32), np.ascontiguousarray(w).view(np.uint32)
        if not np.array_equal(gb, wb):
            at = np.argwhere(gb != wb)
            return f"{name}: {at.shape[0]} words differ, the first at {tuple(at[0])}: {g[tuple(at[0])]!r} against {w[tuple(at[0])]!r}"
    return ""
