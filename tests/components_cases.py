"""TEST INFRASTRUCTURE ONLY -- volumes with known connected components and numpy restatements of what the definition of
vr_label_components claims about the mesh, shared by tests/test_components_cpu.py and tests/test_components_gpu.py.
Volumes are [z, y, x]; a voxel is "inside" where it is 200 and the tests label at iso 100."""
from __future__ import annotations

import numpy as np

DIRS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]                 # adjacent (x, y, z)
NON_ADJACENT = [(1, -1, 0), (1, 0, -1), (0, 1, -1), (1, 1, -1), (1, -1, 1), (-1, 1, 1)]              # of the 26, not of the 14
ON, ISO = 200, 100


def pair_volume(e, dtype=np.uint8):
    """two voxels, A and A + e, alone in 5 x 5 x 5"""
    vol = np.zeros((5, 5, 5), dtype=dtype)
    vol[2, 2, 2] = ON
    vol[2 + e[2], 2 + e[1], 2 + e[0]] = ON
    return vol


def nested_shells(n=33, dtype=np.uint8):
    """a ball (d <= 5) inside a hollow sphere (10 <= d <= 12): two components; the shell holds the lowest voxel, so it is number 1"""
    c = n // 2
    z, y, x = np.mgrid[0:n, 0:n, 0:n]
    d2 = (x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2
    vol = np.zeros((n, n, n), dtype=dtype)
    vol[(d2 <= 25) | ((d2 >= 100) & (d2 <= 144))] = ON
    return vol


def serpentine(n=40, dtype=np.uint8):
    """a one-voxel-wide path through every second row of every second plane of n^3 (n even), joined at alternating ends.
    Returns (volume, length)."""
    assert n % 2 == 0
    vol = np.zeros((n, n, n), dtype=dtype)
    rows = n // 2
    for p in range(n // 2):
        k = 2 * p
        for r in range(rows):
            vol[k, 2 * r, :] = ON
            if r + 1 < rows:
                vol[k, 2 * r + 1, n - 1 if r % 2 == 0 else 0] = ON
        if p + 1 < n // 2:                                  # the path ends where row `rows - 1` ends, or, run backwards, where row 0 began
            end_x = (0 if (rows - 1) % 2 == 1 else n - 1) if p % 2 == 0 else 0
            vol[k + 1, 2 * (rows - 1) if p % 2 == 0 else 0, end_x] = ON
    length = (n // 2) * (rows * n + rows - 1) + n // 2 - 1
    assert int((vol == ON).sum()) == length
    return vol, length


def comb(shape_xyz=(20, 17, 40), dtype=np.uint8):
    """the full plane z = nz - 1 plus columns along z at every third (x, y): the columns' pieces in the tiles below only meet
    through the far plane.  One component.  Returns (volume, voxels)."""
    nx, ny, nz = shape_xyz
    vol = np.zeros((nz, ny, nx), dtype=dtype)
    vol[nz - 1] = ON
    vol[:, 1::3, 1::3] = ON
    return vol, int((vol == ON).sum())


def checkerboard(shape_xyz=(23, 18, 17), dtype=np.uint8):
    """(i + j + k) even: every inside voxel has eight inside neighbours among the 14, none of them along an axis"""
    nx, ny, nz = shape_xyz
    z, y, x = np.mgrid[0:nz, 0:ny, 0:nx]
    return np.where((x + y + z) % 2 == 0, ON, 0).astype(dtype)


def seam_pairs(n=72, boundaries=(4, 8, 16, 32, 64), dtype=np.uint8):
    """n^3 zeros with one voxel pair (A, A + e) per (e in DIRS + NON_ADJACENT) x axis x boundary that straddles the boundary
    between positions b - 1 | b along that axis (e needs a step along the axis), every pair at Chebyshev distance >= 3 from every
    other.  Returns (volume, components): an adjacent pair is one component, a non-adjacent one two."""
    vol = np.zeros((n, n, n), dtype=dtype)
    placed = []                                             # voxels (x, y, z)
    components = 0
    spots = [(u, v) for v in range(2, n - 2, 4) for u in range(2, n - 2, 4)]
    for t, e in enumerate(DIRS + NON_ADJACENT):
        for axis in range(3):
            if e[axis] == 0:
                continue
            for b in boundaries:
                for u, v in spots:
                    a = [0, 0, 0]
                    a[axis] = b - 1 if e[axis] > 0 else b
                    a[(axis + 1) % 3], a[(axis + 2) % 3] = u, v
                    pair = [tuple(a), (a[0] + e[0], a[1] + e[1], a[2] + e[2])]
                    if all(max(abs(p[0] - q[0]), abs(p[1] - q[1]), abs(p[2] - q[2])) >= 3 for p in pair for q in placed):
                        break
                else:
                    raise AssertionError("no room for a pair")
                assert {pair[0][axis], pair[1][axis]} == {b - 1, b}
                for p in pair:
                    vol[p[2], p[1], p[0]] = ON
                placed += pair
                components += 1 if t < len(DIRS) else 2
    return vol, components


CHUNK = 8192                                                # voxels, in linear order, that one workgroup of the records pass folds
REC_SLOTS = 1024                                            # labels its table holds; a run of a further label goes straight to memory
TILE = (32, 8, 4)                                           # the tile pass's tile (x, y, z)


def lattice(shape_xyz, dtype=np.uint8):
    """(x + y + z) % 4 == 0.  Each of the seven directions changes x + y + z by 1, 2 or 3, so no two lattice voxels are adjacent:
    every one is its own component, a quarter of all voxels -- 2048 labels in each full 8192-voxel chunk."""
    nx, ny, nz = shape_xyz
    z, y, x = np.mgrid[0:nz, 0:ny, 0:nx]
    return np.where((x + y + z) % 4 == 0, ON, 0).astype(dtype)


def first_n_per_chunk(mask: np.ndarray, n, chunk=CHUNK):
    """`mask` (a volume; set = non-zero) with only the first n set voxels, in linear order, of every `chunk` consecutive voxels"""
    flat = mask.reshape(-1)
    on = np.zeros(-(-flat.size // chunk) * chunk, dtype=np.int64)
    on[:flat.size] = flat != 0
    rank = np.cumsum(on.reshape(-1, chunk), axis=1).reshape(-1)[:flat.size]      # 1-based among its chunk's set voxels
    return np.where((flat != 0) & (rank <= n), flat, 0).astype(mask.dtype).reshape(mask.shape)


def y_lines(shape_xyz=(4096, 2, 4), dtype=np.uint8):
    """x even and z even, every y: with ny = 2 each (x, z) column is a two-voxel component whose voxels are nx apart in linear
    order -- two separate runs, and with nx * ny = 8192 both in the same chunk"""
    nx, ny, nz = shape_xyz
    vol = np.zeros((nz, ny, nx), dtype=dtype)
    vol[0::2, :, 0::2] = ON
    return vol


def solid_with_hole(shape_xyz=(70, 66, 68), second_block=False, dtype=np.uint8):
    """everything inside except the box x in [10, 60), y in [20, 40), z in [30, 34): one component whose box is the volume and
    whose surface is the hole's.  second_block: a second cavity x in [3, 67), y in [5, 61), z in [40, 64) that holds, one voxel
    clear of its walls all round, a solid block of its own -- two components, whole tiles in each, the surface still closed."""
    nx, ny, nz = shape_xyz
    vol = np.full((nz, ny, nx), ON, dtype=dtype)
    vol[30:34, 20:40, 10:60] = 0
    if second_block:
        assert nx >= 70 and ny >= 66 and nz >= 68
        vol[40:64, 5:61, 3:67] = 0
        vol[42:62, 7:59, 5:65] = ON
    return vol


def lattice_under_a_slab(stem_from, shape_xyz=(64, 16, 24), dtype=np.uint8):
    """one-voxel components and one large one in the same chunk: the lattice in the rows y < 12 of the planes z < 8 (192 a plane,
    1536 in the first chunk), every plane z >= 10 solid, and a stem -- the rows y >= 13 of the planes stem_from <= z < 10 -- that
    brings the slab's component down into the first chunk.  Row 12 keeps the stem clear of the lattice.  With stem_from = 0 the
    large component's first run comes before the first chunk's 1024th label, with stem_from = 6 after its 1344th."""
    nx, ny, nz = shape_xyz
    vol = np.zeros((nz, ny, nx), dtype=dtype)
    vol[:8, :12] = lattice((nx, 12, 8), dtype)
    vol[10:] = ON
    vol[stem_from:10, 13:] = ON
    return vol


def labels_per_chunk(labels: np.ndarray, chunk=CHUNK) -> np.ndarray:
    """the number of distinct non-zero labels in every `chunk` consecutive entries of the flat label array"""
    flat = labels.reshape(-1)
    return np.array([np.count_nonzero(np.unique(flat[at:at + chunk])) for at in range(0, flat.size, chunk)], dtype=np.int64)


def full_tiles(inside: np.ndarray, tile=TILE) -> int:
    """the number of tile-aligned tiles (x, y, z) that lie wholly in the volume [z, y, x] and are all inside"""
    tx, ty, tz = tile
    nz, ny, nx = inside.shape
    mz, my, mx = nz // tz, ny // ty, nx // tx
    whole = np.asarray(inside, dtype=bool)[:mz * tz, :my * ty, :mx * tx].reshape(mz, tz, my, ty, mx, tx)
    return int(whole.all(axis=(1, 3, 5)).sum())


def vertex_labels(inside: np.ndarray, labels: np.ndarray) -> np.ndarray:
    """The extraction's vertex list restated in numpy: for each direction d the voxel pairs (A, A + e_d) with differing inside
    bits, in the order (owner A's linear index, d).  Returns each vertex's label: that of its inside endpoint."""
    nz, ny, nx = inside.shape
    keys, labs = [], []
    lin = np.arange(inside.size, dtype=np.int64).reshape(inside.shape)
    for d, (dx, dy, dz) in enumerate(DIRS):
        a = (slice(0, nz - dz), slice(0, ny - dy), slice(0, nx - dx))
        b = (slice(dz, nz), slice(dy, ny), slice(dx, nx))
        differ = inside[a] != inside[b]
        keys.append(lin[a][differ] * 7 + d)
        labs.append(np.where(inside[a], labels[a], labels[b])[differ])
    keys, labs = np.concatenate(keys), np.concatenate(labs)
    out = labs[np.argsort(keys, kind="stable")].astype(np.uint32)
    assert np.all(out != 0)
    return out


def sub_mesh(mesh, vlabel: np.ndarray, selected: np.ndarray):
    """the kept rows of a full mesh: vertices whose component is selected, triangles of kept vertices, indices renumbered by a
    cumulative sum"""
    pos, nrm, tri = mesh
    keep_v = np.asarray(selected, dtype=bool)[vlabel.astype(np.int64) - 1] if vlabel.size else np.zeros(0, dtype=bool)
    keep_t = keep_v[tri[:, 0].astype(np.int64)] if tri.size else np.zeros(0, dtype=bool)
    new = (np.cumsum(keep_v) - 1).astype(np.uint32)
    return pos[keep_v], nrm[keep_v], new[tri[keep_t].astype(np.int64)].reshape(-1, 3)


def renumber_by_first_voxel(lab: np.ndarray) -> np.ndarray:
    """any labelling (0 = outside) renumbered 1 .. n by ascending first voxel in linear order"""
    flat = lab.reshape(-1)
    ids, first = np.unique(flat, return_index=True)
    first, ids = first[ids != 0], ids[ids != 0]
    table = np.zeros(int(flat.max(initial=0)) + 1, dtype=np.uint32)
    table[ids[np.argsort(first)]] = np.arange(1, ids.size + 1, dtype=np.uint32)
    return table[flat].reshape(lab.shape)
