"""Isosurface extraction without a GPU: the C ABI's new entry points, what a host-only handle answers, and known answers of the
CPU definition (tests/mesh_ref/mesh_ref.c), which tests/test_mesh_gpu.py holds the kernels to.  The known answers are what
keep the restatement from being its own yardstick: counts, closedness, Euler characteristic, exact volumes and areas."""
import ctypes as C
import importlib.util
from pathlib import Path

import numpy as np
import pytest

_HERE = Path(__file__).resolve().parent


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


mesh_ref = _load("mesh_ref_binding", _HERE / "mesh_ref" / "binding.py")
M = _load("mesh_checks", _HERE / "mesh_checks.py")

SYMBOLS = ("vr_extract_isosurface", "vr_get_mesh_info", "vr_read_mesh", "vr_save_mesh", "vr_free_mesh", "vr_set_mesh_workspace",
           "vr_get_mesh_ms")


@pytest.fixture(scope="module")
def meshlib(tmp_path_factory):
    return mesh_ref.build(tmp_path_factory.mktemp("mesh_ref"))


@pytest.mark.parametrize("name", SYMBOLS)
def test_library_exports_the_mesh_entry_points(vra, name):
    assert name in vra.symbols_declared_in_header()
    assert hasattr(C.CDLL(str(vra.LIB_PATH)), name)


def test_host_only_handle_refuses_extraction_and_has_no_mesh(vra, tmp_path):
    R = vra.renderer
    r = vra.RendererCore(-1)
    r.setup((64, 64))
    with pytest.raises(vra.VRError) as e:
        r.extractIsosurface(100)
    assert e.value.code == R.VR_E_NO_DEVICE
    for call in (r.meshInfo, r.readMesh, lambda: r.saveMesh(tmp_path / "m.stl", "stl"), lambda: r.saveMesh(tmp_path / "m.ply", "ply")):
        with pytest.raises(vra.VRError) as e:
            call()
        assert e.value.code == R.VR_E_INVALID
    assert not (tmp_path / "m.stl").exists() and not (tmp_path / "m.ply").exists()
    r.setMeshWorkspace(1 << 20)
    r.freeMesh()                                          # nothing to free is not an error
    assert r.meshMs() == 0.0
    r.close()


@pytest.mark.parametrize("spacing", [(1.0, 1.0, 1.0), (0.5, 1.0, 2.0)])
def test_single_bright_voxel(meshlib, spacing):
    vol = np.zeros((5, 5, 5), dtype=np.uint8)
    vol[2, 2, 2] = 100
    pos, nrm, tri = mesh_ref.extract(meshlib, vol, 50.0, spacing)
    assert pos.shape == (14, 3) and tri.shape == (24, 3)          # one vertex per direction and sign; 24 tetrahedra meet at a voxel
    assert M.closed_and_oriented(tri) == ""
    assert M.every_vertex_referenced(14, tri)
    assert M.euler_characteristic(14, tri) == 2
    assert M.signed_volume(pos, tri) == 0.5 * spacing[0] * spacing[1] * spacing[2]   # exactly; positive: outward winding
    # the gradient is zero at both ends of the eight diagonal edges (central differences): step 5 gives (0, 0, 0) there; the six
    # axis edges carry unit normals out of the bright voxel
    length = np.linalg.norm(nrm.astype(np.float64), axis=1)
    assert sorted(length.tolist()) == [0.0] * 8 + [1.0] * 6
    centre = np.array([2.0, 2.0, 2.0]) * np.array(spacing)
    out = np.einsum("ij,ij->i", nrm.astype(np.float64), pos.astype(np.float64) - centre)
    assert np.all(out[length == 1.0] > 0)


def test_ramp_along_x_is_a_flat_sheet(meshlib):
    nx, ny, nz = 6, 5, 4
    vol = np.broadcast_to((10 * np.arange(nx)).astype(np.uint8)[None, None, :], (nz, ny, nx)).copy()
    pos, nrm, tri = mesh_ref.extract(meshlib, vol, 25.0, (0.5, 2.0, 3.0))
    assert pos.shape == (63, 3) and tri.shape == (96, 3)
    assert np.all(pos[:, 0] == np.float32(1.25))
    cr = M.cross_products(pos, tri)
    assert np.all(cr[:, 0] < 0) and np.all(cr[:, 1:] == 0)        # every triangle faces -x, the side of the lower values
    assert 0.5 * np.abs(cr[:, 0]).sum() == 72.0                   # 4 x 2 by 3 x 3, exactly
    assert np.array_equal(nrm, np.broadcast_to(np.array([-1.0, 0.0, 0.0], dtype=np.float32), (63, 3)))
    assert M.every_vertex_referenced(63, tri)


@pytest.mark.parametrize("iso_s", [9000.0, 30000.0, 60000.0])
def test_noise_inside_a_zero_border_gives_a_closed_oriented_surface(meshlib, iso_s):
    rng = np.random.default_rng(11)
    vol = np.zeros((10, 11, 12), dtype=np.uint16)
    vol[1:-1, 1:-1, 1:-1] = rng.integers(0, 65536, size=(8, 9, 10))
    pos, nrm, tri = mesh_ref.extract(meshlib, vol, iso_s, (1.0, 0.7, 1.3))
    assert tri.shape[0] > 100
    assert M.closed_and_oriented(tri) == ""
    assert M.every_vertex_referenced(pos.shape[0], tri)
    assert M.signed_volume(pos, tri) > 0
    assert np.all(np.isfinite(pos)) and np.all(np.isfinite(nrm))


def test_digitised_sphere(meshlib):
    n = 24
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64),) * 3, indexing="ij")
    d = np.sqrt((x - 11.3) ** 2 + (y - 11.6) ** 2 + (z - 12.1) ** 2)
    vol = np.clip(np.rint(128.0 + 30.0 * (8.2 - d)), 0, 255).astype(np.uint8)
    pos, nrm, tri = mesh_ref.extract(meshlib, vol, 128.0)
    assert M.closed_and_oriented(tri) == ""
    assert M.euler_characteristic(pos.shape[0], tri) == 2
    volume = M.signed_volume(pos, tri)
    assert 0.9 < volume / (4.0 / 3.0 * np.pi * 8.2 ** 3) < 1.0    # a polyhedron inscribed in the sphere, up to the digitisation
    cr = M.cross_products(pos, tri)
    solid = np.linalg.norm(cr, axis=1) > 0
    assert solid.sum() > 0.9 * tri.shape[0]
    for corner in range(3):                                       # each vertex normal of a triangle lies on its front side
        assert np.all(np.einsum("ij,ij->i", nrm.astype(np.float64)[tri[solid, corner]], cr[solid]) > 0)


def test_winding_check_value(meshlib):
    even = sum(1 << m for m in (2, 5, 8, 10, 11, 14))
    odd = sum(1 << m for m in range(1, 15)) ^ even
    # xyz, xzy, yxz, yzx, zxy, zyx
    assert [meshlib.mesh_case_swapped(t) for t in range(6)] == [even, odd, odd, even, even, odd]


@pytest.mark.parametrize("shape", [(1, 7, 9), (7, 1, 9), (7, 9, 1), (1, 1, 1), (2, 1, 2)])
def test_a_volume_without_cells_gives_an_empty_mesh(meshlib, shape):
    vol = np.random.default_rng(3).integers(0, 256, size=shape).astype(np.uint8)
    pos, nrm, tri = mesh_ref.extract(meshlib, vol, 128.0)
    assert pos.shape == (0, 3) and nrm.shape == (0, 3) and tri.shape == (0, 3)


def test_an_iso_value_outside_the_data_gives_an_empty_mesh(meshlib):
    vol = np.random.default_rng(4).integers(100, 200, size=(6, 7, 8)).astype(np.uint16)
    lo, hi = int(vol.min()), int(vol.max())
    for iso_s in (float(lo), float(lo - 50), float(hi + 1), 70000.0, -5.0):   # every voxel inside; every voxel outside
        pos, nrm, tri = mesh_ref.extract(meshlib, vol, iso_s)
        assert pos.shape[0] == 0 and tri.shape[0] == 0, iso_s
    pos, nrm, tri = mesh_ref.extract(meshlib, vol, float(hi))     # the maximum alone is inside
    assert tri.shape[0] > 0


def test_a_voxel_equal_to_iso_gives_f_zero_and_no_nan(meshlib):
    vol = np.random.default_rng(5).integers(0, 5, size=(7, 8, 9)).astype(np.uint8)
    pos, nrm, tri = mesh_ref.extract(meshlib, vol, 2.0, (1.0, 1.0, 1.0))
    assert tri.shape[0] > 0
    assert np.all(np.isfinite(pos)) and np.all(np.isfinite(nrm))
    on_lattice = np.all(pos == np.rint(pos), axis=1)              # f == 0: the vertex is the voxel whose value is iso
    assert on_lattice.sum() > 0
    ijk = pos[on_lattice].astype(np.int64)
    assert np.all(vol[ijk[:, 2], ijk[:, 1], ijk[:, 0]] == 2)
    area = np.linalg.norm(M.cross_products(pos, tri), axis=1)
    assert (area == 0).sum() > 0                                   # coinciding vertices: zero-area triangles, kept
    assert M.every_vertex_referenced(pos.shape[0], tri)


def test_box_extraction_is_the_whole_mesh_when_the_rest_is_empty(meshlib):
    rng = np.random.default_rng(6)
    vol = np.zeros((9, 12, 14), dtype=np.uint8)
    vol[5:, 7:, 8:] = rng.integers(0, 256, size=(4, 5, 6))         # a block in the last corner
    whole = mesh_ref.extract(meshlib, vol, 100.0, (0.5, 1.0, 2.0))
    box = mesh_ref.extract(meshlib, vol, 100.0, (0.5, 1.0, 2.0), box=((7, 6, 4), (13, 11, 8)))
    assert whole[2].shape[0] > 0 and M.same_bits(box, whole) == ""
