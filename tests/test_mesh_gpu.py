"""vr_extract_isosurface on the device against its CPU definition (tests/mesh_ref/mesh_ref.c), bit for bit as arrays: both voxel
types, both layouts, shapes that are no multiple of a brick, one cell thick or without cells; z slabs; the smoothed volume; that
the mesh is a snapshot and an extraction leaves every rendering state alone; the mesh's own properties without the restatement;
the STL and PLY files; and a volume beyond 2^32 bytes."""
import ctypes as C
import importlib.util
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_HERE = Path(__file__).resolve().parent


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


mesh_ref = _load("mesh_ref_binding", _HERE / "mesh_ref" / "binding.py")
smooth_ref = _load("smooth_ref_binding", _HERE / "smooth_ref" / "binding.py")
M = _load("mesh_checks", _HERE / "mesh_checks.py")

SHAPES = [(13, 11, 6), (70, 66, 68), (5, 3, 2), (64, 2, 2), (5, 3, 1)]          # (nx, ny, nz); the last has no cells
ISOS = {np.uint8: (40, 128, 220), np.uint16: (8000, 30000, 60000)}
SPACING = (0.5, 1.0, 2.0)
LAYOUTS = pytest.mark.parametrize("layout", [0, 1], ids=["linear", "bricked"])
DTYPES = pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])


@pytest.fixture(scope="module")
def meshlib(tmp_path_factory):
    return mesh_ref.build(tmp_path_factory.mktemp("mesh_ref_gpu"))


@pytest.fixture(scope="module")
def handle(vra):
    r = vra.RendererCore(0)
    r.setup((64, 48))
    assert r.loadShader("VolumeRenderer.cs")
    yield r
    r.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def random_volume(shape_xyz, dtype, seed):
    nx, ny, nz = shape_xyz
    hi = 256 if dtype == np.uint8 else 65536
    return np.random.default_rng(seed).integers(0, hi, size=(nz, ny, nx)).astype(dtype)


_REF = {}


def reference(meshlib, key, vol, iso_s, spacing):
    """the CPU definition's mesh, computed once per (volume key, iso_s, spacing) and shared"""
    k = (key, float(iso_s), tuple(spacing))
    if k not in _REF:
        out = mesh_ref.extract(meshlib, vol, iso_s, spacing)
        for a in out:
            a.setflags(write=False)
        _REF[k] = out
    return _REF[k]


def assert_same_mesh(got, want, what):
    problem = M.same_bits(got, want)
    assert not problem, f"{what}: {problem}"


@DTYPES
@LAYOUTS
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_read_mesh_matches_the_reference(vra, meshlib, handle, shape, layout, dtype):
    R = vra.renderer
    r = handle
    seed = sum(shape) + np.dtype(dtype).itemsize
    vol = random_volume(shape, dtype, seed)
    r.setLayout(layout)
    r.setQuirks(R.QUIRK_DEFAULT)
    r.setVolume(vol, SPACING)
    cells = min(shape) >= 2
    for iso in ISOS[dtype]:
        iso_s = mesh_ref.iso_stored(iso, dtype, True)
        nv, nt = r.extractIsosurface(iso)
        want = reference(meshlib, (shape, seed), vol, iso_s, SPACING)
        assert (nv, nt) == (want[0].shape[0], want[2].shape[0]) and (nt > 0) == cells
        assert r.meshInfo() == dict(iso=iso, vertices=nv, triangles=nt)
        assert_same_mesh(r.readMesh(), want, f"iso {iso}")
    if dtype == np.uint16:                                  # without the quirk the same number means another surface
        r.setQuirks(0)
        iso = ISOS[dtype][1]
        r.extractIsosurface(iso)
        assert_same_mesh(r.readMesh(), reference(meshlib, (shape, seed), vol, float(iso), SPACING), "quirk off")
        if cells:
            assert M.same_bits(r.readMesh(), reference(meshlib, (shape, seed), vol, float(iso + 1000), SPACING)) != ""
        r.setQuirks(R.QUIRK_DEFAULT)


@LAYOUTS
def test_full_range_u16_with_the_extremes_at_the_corners(vra, meshlib, handle, layout):
    r = handle
    shape = (13, 11, 6)
    vol = random_volume(shape, np.uint16, 99)
    vol[0, 0, 0] = 0; vol[-1, -1, -1] = 65535; vol[0, 0, -1] = 65535; vol[-1, -1, 0] = 0; vol[0, -1, 0] = 65535; vol[-1, 0, -1] = 0
    r.setLayout(layout)
    r.setQuirks(0)
    r.setVolume(vol, (1.0, 1.0, 1.0))
    for iso in (1, 32768, 65535):                           # the lowest and the highest value that still give a surface
        r.extractIsosurface(iso)
        got = r.readMesh()
        assert got[2].shape[0] > 0
        assert_same_mesh(got, reference(meshlib, ("full", 99), vol, float(iso), (1.0, 1.0, 1.0)), f"iso {iso}")
    assert r.extractIsosurface(65536) == (0, 0) and r.extractIsosurface(0) == (0, 0) and r.extractIsosurface(-7) == (0, 0)
    r.setQuirks(vra.renderer.QUIRK_DEFAULT)


@DTYPES
@LAYOUTS
def test_z_slabs_give_the_same_bytes_as_one_piece(vra, meshlib, handle, layout, dtype):
    r = handle
    shape = (70, 66, 68)
    seed = sum(shape) + np.dtype(dtype).itemsize
    vol = random_volume(shape, dtype, seed)
    r.setLayout(layout)
    r.setVolume(vol, SPACING)
    iso = ISOS[dtype][1]
    r.setMeshWorkspace(0)
    r.extractIsosurface(iso)
    whole = r.readMesh()
    assert_same_mesh(whole, reference(meshlib, (shape, seed), vol, mesh_ref.iso_stored(iso, dtype), SPACING), "one piece")
    plane = 9 * shape[0] * shape[1]                        # the work arrays' bytes per plane
    try:
        for planes in (2, 3, 8, 67):                       # slabs of 1, 2, 7 and 66 planes: 68, 34, 10 and 2 of them
            r.setMeshWorkspace(planes * plane + plane // 2)
            assert r.extractIsosurface(iso) == (whole[0].shape[0], whole[2].shape[0])
            assert_same_mesh(r.readMesh(), whole, f"{planes} planes of work arrays")
    finally:
        r.setMeshWorkspace(0)


def test_the_mesh_is_that_of_the_smoothed_volume(vra, oracle, meshlib, handle):
    r = handle
    R = vra.renderer
    vol = oracle.gen_noise_ball((41, 39, 40), 2, 77)
    r.setLayout(R.LAYOUT_BRICKED)
    r.setVolume(vol, SPACING)
    iso = (int(vol.min()) + int(vol.max())) // 2 - 1000
    r.extractIsosurface(iso)
    loaded = r.readMesh()
    assert_same_mesh(loaded, reference(meshlib, "ball16", vol, float(iso + 1000), SPACING), "as loaded")
    r.smoothVolume(sigma_voxels=(1.0, 1.0, 1.0))
    assert_same_mesh(r.readMesh(), loaded, "the snapshot after smoothing")
    smoothed = r.readVolume()
    assert not np.array_equal(smoothed, vol)
    r.extractIsosurface(iso)
    got = r.readMesh()
    assert got[2].shape[0] > 0 and M.same_bits(got, loaded) != ""
    assert_same_mesh(got, mesh_ref.extract(meshlib, smoothed, float(iso + 1000), SPACING), "smoothed")
    r.smoothVolume(sigma_voxels=0.0)
    r.extractIsosurface(iso)
    assert_same_mesh(r.readMesh(), loaded, "after (0, 0, 0)")


MODES = ["composite", "mip", "trilinear", "iso", "shade", "reslice"]


def set_mode(vra, r, mode, dims):
    R = vra.renderer
    r.setIsosurface(False)
    r.setReslice(False)
    r.setShading(False)
    r.setMIP(mode == "mip")
    r.setFilter(R.FILTER_TRILINEAR if mode == "trilinear" else R.FILTER_NEAREST)
    if mode == "iso":
        r.setIsosurface(True, 120)
    elif mode == "shade":
        r.setShading(True, 0.2, 0.7, 0.3, 8)
    elif mode == "reslice":
        r.setReslice(True, vra.axis_reslice(2, dims[2] // 2, dims, (1.0, 1.0, 1.0), r.framebuffer_size, n=5), mode="mean", n=5)


def frame(r):
    r.render()
    rgba = r.readPixels().copy()
    total, spp = r.countSamples(per_pixel=True)
    return rgba, spp.copy(), total


def test_the_mesh_is_a_snapshot_and_an_extraction_leaves_the_renderer_alone(vra, oracle, meshlib, handle):
    r = handle
    R = vra.renderer
    dims = (41, 39, 40)
    vol = oracle.gen_noise_ball(dims, 1, 77)
    r.setLayout(R.LAYOUT_BRICKED)
    r.setVolume(vol)
    r.setWindow(20, 230)
    r.setAlpha(0.3)
    r.freeMesh()
    with pytest.raises(vra.VRError) as e:
        r.readMesh()
    assert e.value.code == R.VR_E_INVALID
    before = {}
    for m in MODES:
        set_mode(vra, r, m, dims)
        before[m] = frame(r)
    r.takeMessage()
    state = (r.window, r.residentBytes()[:2], bits(r.getCameraBlock()).tolist(), r.smoothing)
    other, choice, kernel = r.residentBytes()[2], r.last_launch_choice, r.last_kernel_name
    nv, nt = r.extractIsosurface(120)
    assert nt > 0 and r.takeMessage() is None
    assert (r.last_launch_choice, r.last_kernel_name) == (choice, kernel)
    assert r.meshMs() > 0.0
    assert (r.window, r.residentBytes()[:2], bits(r.getCameraBlock()).tolist(), r.smoothing) == state
    assert r.residentBytes()[2] == other + 24 * nv + 12 * nt              # the mesh counts under `other`
    mesh = r.readMesh()
    assert_same_mesh(mesh, reference(meshlib, "ball8", vol, 120.0, (1.0, 1.0, 1.0)), "noise ball")
    for m in MODES:
        set_mode(vra, r, m, dims)
        got = frame(r)
        assert np.array_equal(bits(got[0]), bits(before[m][0])), f"{m}: the frame changed"
        assert np.array_equal(got[1], before[m][1]) and got[2] == before[m][2], f"{m}: sample counts changed"
    set_mode(vra, r, "composite", dims)
    # a refused extraction (work arrays bounded below two planes) leaves the mesh
    r.setMeshWorkspace(100)
    with pytest.raises(vra.VRError) as e:
        r.extractIsosurface(60)
    assert e.value.code == R.VR_E_NOMEM
    r.setMeshWorkspace(0)
    assert r.meshInfo() == dict(iso=120, vertices=nv, triangles=nt)
    assert_same_mesh(r.readMesh(), mesh, "after a refused extraction")
    # ... and so does loading another volume
    r.setVolume(random_volume((9, 8, 7), np.uint16, 1))
    assert_same_mesh(r.readMesh(), mesh, "after setVolume")
    lib = vra.load_library()
    assert lib.vr_read_mesh(r._h, None, None, None, 0, 0) == R.VR_OK          # every pointer may be NULL
    small = np.zeros((nv - 1, 3), dtype=np.float32)
    assert lib.vr_read_mesh(r._h, small.ctypes.data_as(C.POINTER(C.c_float)), None, None, nv - 1, nt) == R.VR_E_INVALID
    r.freeMesh()
    assert r.residentBytes()[2] == other
    with pytest.raises(vra.VRError):
        r.meshInfo()
    fresh = vra.RendererCore(0)
    try:
        fresh.setup((64, 48))
        with pytest.raises(vra.VRError) as e:
            fresh.extractIsosurface(100)                    # before any volume: what vr_read_volume gives
        assert e.value.code == R.VR_E_INVALID
    finally:
        fresh.close()


def zero_bordered_noise(dtype=np.uint16):
    rng = np.random.default_rng(11)
    vol = np.zeros((20, 23, 26), dtype=dtype)
    vol[1:-1, 1:-1, 1:-1] = rng.integers(0, 65536 if dtype == np.uint16 else 256, size=(18, 21, 24))
    return vol


@LAYOUTS
def test_the_gpu_mesh_is_closed_and_consistently_oriented(vra, handle, layout):
    """in numpy alone: no restatement involved"""
    r = handle
    r.setLayout(layout)
    r.setQuirks(0)
    r.setVolume(zero_bordered_noise(), (1.0, 0.7, 1.3))
    try:
        for iso in (9000, 30000, 60000):
            r.extractIsosurface(iso)
            pos, nrm, tri = r.readMesh()
            assert tri.shape[0] > 1000
            assert M.closed_and_oriented(tri) == ""
            assert M.every_vertex_referenced(pos.shape[0], tri)
            assert M.signed_volume(pos, tri) > 0
            assert np.all(np.isfinite(pos)) and np.all(np.isfinite(nrm))
            length = np.linalg.norm(nrm.astype(np.float64), axis=1)
            assert np.all((length == 0) | (np.abs(length - 1.0) < 1e-6))
    finally:
        r.setQuirks(vra.renderer.QUIRK_DEFAULT)


def test_stl_and_ply_files(vra, handle, tmp_path):
    r = handle
    R = vra.renderer
    vol = np.random.default_rng(5).integers(0, 5, size=(7, 8, 9)).astype(np.uint8)       # voxels equal to iso: zero-area triangles
    r.setLayout(R.LAYOUT_BRICKED)
    r.setVolume(vol, SPACING)
    nv, nt = r.extractIsosurface(2)
    pos, nrm, tri = r.readMesh()
    for bad in ("obj", ".stl", "STL", ""):
        with pytest.raises(vra.VRError) as e:
            r.saveMesh(tmp_path / "bad", bad)
        assert e.value.code == R.VR_E_INVALID
    assert not (tmp_path / "bad").exists()
    with pytest.raises(vra.VRError) as e:
        r.saveMesh(tmp_path / "no_such_directory" / "m.stl", "stl")
    assert e.value.code == R.VR_E_IO

    r.saveMesh(tmp_path / "m.stl", "stl")
    raw = (tmp_path / "m.stl").read_bytes()
    assert len(raw) == 84 + 50 * nt and not raw.startswith(b"solid")
    assert int(np.frombuffer(raw, dtype="<u4", count=1, offset=80)[0]) == nt
    rec = np.frombuffer(raw, dtype=np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("a", "<u2")]), offset=84)
    assert rec.shape == (nt,) and np.all(rec["a"] == 0)
    assert np.array_equal(rec["v"].view(np.uint32), pos[tri.astype(np.int64)].view(np.uint32))
    cr = M.cross_products(pos, tri)
    flat = np.all(cr == 0, axis=1)
    assert flat.sum() > 0 and (~flat).sum() > 0
    assert np.all(rec["n"][flat] == 0)
    assert np.all(np.einsum("ij,ij->i", rec["n"][~flat].astype(np.float64), cr[~flat]) > 0)
    assert np.allclose(np.linalg.norm(rec["n"][~flat].astype(np.float64), axis=1), 1.0, atol=1e-6)

    r.saveMesh(tmp_path / "m.ply", "ply")
    raw = (tmp_path / "m.ply").read_bytes()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0" and lines[-1] == "end_header"
    lines = [ln for ln in lines if not ln.startswith("comment")]
    assert lines[2:] == [f"element vertex {nv}"] + [f"property float {p}" for p in ("x", "y", "z", "nx", "ny", "nz")] + \
        [f"element face {nt}", "property list uchar uint vertex_indices", "end_header"]
    assert len(raw) == end + 24 * nv + 13 * nt
    verts = np.frombuffer(raw, dtype="<f4", count=6 * nv, offset=end).reshape(nv, 6)
    assert np.array_equal(verts[:, :3].view(np.uint32), pos.view(np.uint32)) and np.array_equal(verts[:, 3:].view(np.uint32), nrm.view(np.uint32))
    faces = np.frombuffer(raw, dtype=np.dtype([("n", "u1"), ("i", "<u4", 3)]), offset=end + 24 * nv)
    assert np.all(faces["n"] == 3) and np.array_equal(faces["i"], tri)


def test_a_volume_beyond_2_to_the_32_bytes(vra, meshlib):
    """u8, 1024 x 1024 x 4100 (4.0 GiB + 4 planes), zeros but a random 24^3 block in the last planes, in each layout.  The work
    arrays of the default bound hold 227 planes, so the extraction runs in 19 slabs; the block lies in the last one and
    straddles the voxel offset 2^32 (plane 4096).  The mesh equals the restatement's extraction of that corner's cells: no voxel outside them owns a vertex."""
    R = vra.renderer
    nx, ny, nz, b = 1024, 1024, 4100, 24
    vol = np.zeros((nz, ny, nx), dtype=np.uint8)
    vol[nz - b:, ny - b:, nx - b:] = np.random.default_rng(2).integers(0, 256, size=(b, b, b))
    assert (nz - b) * ny * nx < 2 ** 32 < (nz - 1) * ny * nx
    want = mesh_ref.extract(meshlib, vol, 128.0, SPACING, box=((nx - b - 1, ny - b - 1, nz - b - 1), (nx - 1, ny - 1, nz - 1)))
    assert want[2].shape[0] > 10000
    r = vra.RendererCore(0)
    try:
        r.setup((64, 48))
        assert r.loadShader("VolumeRenderer.cs")
        r.setLayout(R.LAYOUT_LINEAR)
        r.setVolume(vol, SPACING)
        for layout in (R.LAYOUT_LINEAR, R.LAYOUT_BRICKED):
            r.setLayout(layout)
            r.freeMesh()
            assert r.extractIsosurface(128) == (want[0].shape[0], want[2].shape[0])
            assert_same_mesh(r.readMesh(), want, f"layout {layout}")
    finally:
        r.close()
