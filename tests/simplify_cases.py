"""TEST INFRASTRUCTURE ONLY -- shared by tests/test_simplify_cpu.py and tests/test_simplify_gpu.py: an independent numpy statement of
vr_simplify_mesh's definition (include/vr_core.h), the consequences of its step 6 as checks on any (input, output) pair, and the
volumes whose meshes both files simplify.  Nothing here knows how a simplification was computed."""
from __future__ import annotations

import numpy as np

CELLS = (0.3, 1.5, 4.0, 8.0, 1000.0)
SPACING = (0.5, 1.0, 2.0)
MAX_QUOTIENT = np.float32(2097152.0)


def cells_of(pos: np.ndarray, cell) -> np.ndarray:
    """step 2: [nv, 3] int64 cell indices; OverflowError where a quotient is not in [0, 2^21)"""
    q = pos.astype(np.float32) / np.float32(cell)
    assert q.dtype == np.float32
    if not np.all((q >= np.float32(0.0)) & (q < MAX_QUOTIENT)):
        raise OverflowError("a quotient is not in [0, 2^21)")
    return np.floor(q).astype(np.int64)


def key_bits(pos: np.ndarray, cell) -> list:
    """[bx, by, bz]: the bits the largest cell index on each axis needs -- the widths of the three fields an implementation may
    pack into one sort key (0: every vertex is in cell 0 on that axis)"""
    return [int(m).bit_length() for m in cells_of(pos, cell).max(axis=0)]


def numpy_simplify(mesh, cell):
    """the definition with lexsort and unique: returns ((positions, normals, triangles), rows)"""
    pos, nrm, tri = mesh
    cell = np.float32(cell)
    nv = pos.shape[0]
    if nv == 0 or tri.shape[0] == 0:
        return (pos[:0].copy(), nrm[:0].copy(), tri[:0].copy()), np.zeros(0, dtype=np.uint32)
    c = cells_of(pos, cell)
    centre = (c.astype(np.float32) + np.float32(0.5)) * cell
    d = pos - centre
    zz, yy, xx = d[:, 2] * d[:, 2], d[:, 1] * d[:, 1], d[:, 0] * d[:, 0]
    dist = (zz + yy) + xx
    assert centre.dtype == np.float32 and dist.dtype == np.float32
    key = c[:, 0] | c[:, 1] << 21 | c[:, 2] << 42
    order = np.lexsort((np.arange(nv), dist.view(np.uint32), key))          # by key, then dist, then index
    ks = key[order]
    head = np.r_[True, ks[1:] != ks[:-1]]
    first = np.maximum.accumulate(np.where(head, np.arange(nv), 0))
    rep = np.empty(nv, dtype=np.int64)
    rep[order] = order[first]
    m = rep[tri.astype(np.int64)]
    cand = np.flatnonzero((m[:, 0] != m[:, 1]) & (m[:, 1] != m[:, 2]) & (m[:, 0] != m[:, 2]))
    if cand.size == 0:
        return (pos[:0].copy(), nrm[:0].copy(), tri[:0].copy()), np.zeros(0, dtype=np.uint32)
    _, where = np.unique(np.sort(m[cand], axis=1), axis=0, return_index=True)   # the first occurrence of every vertex set
    kept = np.sort(cand[where])
    rows = np.unique(m[kept])
    renumber = np.full(nv, -1, dtype=np.int64)
    renumber[rows] = np.arange(rows.size)
    return (pos[rows], nrm[rows], renumber[m[kept]].astype(np.uint32)), rows.astype(np.uint32)


def consequences(source, result, rows, cell) -> str:
    """'' when `result` (with `rows`, the input index of every output vertex) has the properties step 6 promises of a
    simplification of `source`; else what is wrong"""
    (spos, snrm, _), (pos, nrm, tri) = source, result
    if rows.shape != (pos.shape[0],) or np.any(np.diff(rows.astype(np.int64)) <= 0):
        return "the output rows are not input rows in ascending order"
    if not (np.array_equal(pos.view(np.uint32), spos[rows].view(np.uint32)) and np.array_equal(nrm.view(np.uint32), snrm[rows].view(np.uint32))):
        return "an output vertex is not its input row bit for bit"
    if tri.shape[0] == 0:
        return "" if pos.shape[0] == 0 else "vertices without a triangle"
    if not np.array_equal(np.unique(tri), np.arange(pos.shape[0], dtype=tri.dtype)):
        return "a vertex is not referenced (or an index is out of range)"
    c = cells_of(pos, cell)
    if np.unique(c, axis=0).shape[0] != c.shape[0]:
        return "two output vertices share a cell"
    if np.any((tri[:, 0] == tri[:, 1]) | (tri[:, 1] == tri[:, 2]) | (tri[:, 0] == tri[:, 2])):
        return "a degenerate triangle"
    if np.unique(np.sort(tri, axis=1), axis=0).shape[0] != tri.shape[0]:
        return "two triangles with the same vertex set"
    return ""


# ---------------------------------------------------------------- volumes [z, y, x]
def random_volume(shape_xyz, dtype, seed):
    nx, ny, nz = shape_xyz
    hi = 256 if dtype == np.uint8 else 65536
    return np.random.default_rng(seed).integers(0, hi, size=(nz, ny, nx)).astype(dtype)


def ties_volume(shape_xyz, iso, seed, dtype=np.uint8):
    """values from {iso - 1, iso, iso + 1} only: every edge from a voxel equal to iso has f = 0, so vertices coincide in droves"""
    nx, ny, nz = shape_xyz
    return (np.random.default_rng(seed).integers(-1, 2, size=(nz, ny, nx)) + int(iso)).astype(dtype)


def ball_volume(n=64, radius=24.0):
    """a ball with a soft edge, u8: 128 on the sphere of `radius` about the centre, 8 grey levels a voxel across it"""
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64),) * 3, indexing="ij")
    d = np.sqrt((x - (n - 1) / 2) ** 2 + (y - (n - 1) / 2) ** 2 + (z - (n - 1) / 2) ** 2)
    return np.clip(np.rint(128.0 + 8.0 * (radius - d)), 0, 255).astype(np.uint8)


# ---------------------------------------------------------------- cells that make the packed key wide, or an axis of it empty
# the largest cell on extents of 39 whose largest quotient is still below 2^21: the accepting neighbour of the refusal
LARGEST_KEY_CELL = float(np.float32(39.0) / np.float32(2097151.0))
# name -> (volume, iso, spacing).  The ties volume's thousands of coincident vertices share a cell however small it is.
KEY_VOLUMES = {
    "ties": (lambda: ties_volume((40, 38, 36), 100, 5), 100, (1.0, 1.0, 1.0)),
    "ties, unequal": (lambda: ties_volume((40, 38, 36), 100, 5), 100, SPACING),
    "flat z": (lambda: random_volume((70, 66, 2), np.uint8, 3), 128, (1.0, 1.0, 0.25)),
    "flat x": (lambda: random_volume((2, 66, 70), np.uint8, 3), 128, (0.25, 1.0, 1.0)),
}
# (volume, cell, [bx, by, bz])
KEY_CASES = [
    ("ties", 0.01, [12, 12, 12]),                           # 36 bits: the shifts cross bit 31
    # 39 bits on a power of two: vertices half a voxel apart along z differ only in bit 32 of the key and above, so a key that
    # lost those bits would merge them (at 0.01 the ties volume has no two vertices that only such bits tell apart)
    ("ties", 2.0 ** -7, [13, 13, 13]),
    ("ties", 1e-4, [19, 19, 19]),                           # 57 bits
    ("ties", LARGEST_KEY_CELL, [21, 21, 21]),               # 63 bits: the widest key there is
    ("ties, unequal", 1e-4, [18, 19, 20]),
    ("flat z", 0.3, [8, 8, 0]),                             # no bits for z
    ("flat z", 1.5, [6, 6, 0]),
    ("flat x", 0.3, [0, 8, 8]),                             # no bits for x: y is shifted by 0
    ("flat x", 1.5, [0, 6, 6]),
]
KEY_CASE_IDS = [f"{name}, {sum(bits)} bits" for name, cell, bits in KEY_CASES]


def assert_key_case(pos: np.ndarray, name, cell, bits):
    """the case exists: the vertices `pos` of KEY_VOLUMES[name]'s mesh need exactly `bits` at `cell`"""
    assert key_bits(pos, cell) == bits, (name, cell, key_bits(pos, cell))
    if cell == LARGEST_KEY_CELL:
        assert int(cells_of(pos, cell).max()) < 2 ** 21 and float(pos.max()) == 39.0
        assert np.float32(39.0) / np.float32(cell) > np.float32(2 ** 21 - 2)       # ... and no cell could be smaller by much
