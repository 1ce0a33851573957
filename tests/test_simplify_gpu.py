"""vr_simplify_mesh on the device against its CPU definition (tests/simplify_ref/simplify_ref.c), bit for bit as arrays: the mesh
the device extracted is read back, simplified by the restatement and compared with what the device made of it -- both voxel
types, both layouts, a handful of triangles and a million vertices, coincident vertices, cells so small that the packed sort key
needs up to all of its 63 bits and extents that leave an axis none, smoothed and filtered meshes, repeated
calls, what the call does to the handle's state, what it refuses, and the files written from its result."""
import importlib.util
import struct
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


simp_ref = _load("simplify_ref_binding", _HERE / "simplify_ref" / "binding.py")
M = _load("mesh_checks", _HERE / "mesh_checks.py")
S = _load("simplify_cases", _HERE / "simplify_cases.py")

ISO = {np.uint8: 128, np.uint16: 30000}
CELLS = (0.3, 1.5, 4.0, 1000.0)
LAYOUTS = pytest.mark.parametrize("layout", [0, 1], ids=["linear", "bricked"])
DTYPES = pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])


@pytest.fixture(scope="module")
def simplib(tmp_path_factory):
    return simp_ref.build(tmp_path_factory.mktemp("simplify_ref_gpu"))


@pytest.fixture(scope="module")
def handle(vra):
    r = vra.RendererCore(0)
    r.setup((64, 48))
    assert r.loadShader("VolumeRenderer.cs")
    yield r
    r.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same_mesh(got, want, what):
    problem = M.same_bits(got, want)
    assert not problem, f"{what}: {problem}"


_SOURCE, _REF = {}, {}


def source_and_reference(simplib, r, key, cell):
    """the device's resident (unsimplified) mesh and the restatement's simplification of it.  Both layouts extract the same mesh
    (tests/test_mesh_gpu.py), so it is read and simplified on the CPU once per (key, cell) and the later reader only compares."""
    src = r.readMesh()
    if key not in _SOURCE:
        for a in src:
            a.setflags(write=False)
        _SOURCE[key] = src
    else:
        assert_same_mesh(src, _SOURCE[key], f"{key}: the mesh to simplify")
    if (key, cell) not in _REF:
        want, rows = simp_ref.simplify(simplib, _SOURCE[key], cell)
        for a in want:
            a.setflags(write=False)
        _REF[(key, cell)] = want
    return _SOURCE[key], _REF[(key, cell)]


def simplify_and_compare(simplib, r, key, cell):
    src, want = source_and_reference(simplib, r, key, cell)
    nv, nt = r.simplifyMesh(cell)
    got = r.readMesh()
    assert (nv, nt) == (got[0].shape[0], got[2].shape[0]) == (want[0].shape[0], want[2].shape[0]), f"{key}, cell {cell}"
    assert_same_mesh(got, want, f"{key}, cell {cell}")
    assert r.meshSimplification() == dict(cell=float(np.float32(cell)), source_vertices=src[0].shape[0], source_triangles=src[2].shape[0])
    return src, got


# ---------------------------------------------------------------- 1. shapes and types
@pytest.mark.parametrize("cell", CELLS)
@DTYPES
@LAYOUTS
@pytest.mark.parametrize("shape", [(13, 11, 6), (70, 66, 68)], ids=lambda s: "x".join(map(str, s)))
def test_simplification_matches_the_reference(vra, simplib, handle, shape, layout, dtype, cell):
    r = handle
    seed = sum(shape) + np.dtype(dtype).itemsize
    r.setLayout(layout)
    r.setQuirks(vra.renderer.QUIRK_DEFAULT)
    r.setVolume(S.random_volume(shape, dtype, seed), S.SPACING)
    nv, nt = r.extractIsosurface(ISO[dtype])
    if shape == (70, 66, 68):
        assert nv > 500000                                   # clusters and equal triples straddle the blocks of the sorts and scans
    src, got = simplify_and_compare(simplib, r, (shape, np.dtype(dtype).name), cell)
    assert (got[2].shape[0] == 0) == (cell == 1000.0)
    assert r.meshInfo() == dict(iso=ISO[dtype], vertices=got[0].shape[0], triangles=got[2].shape[0])


@DTYPES
@LAYOUTS
def test_a_handful_of_triangles_and_the_empty_mesh(vra, simplib, handle, layout, dtype):
    r = handle
    r.setLayout(layout)
    r.setQuirks(vra.renderer.QUIRK_DEFAULT)
    for shape in ((5, 3, 2), (5, 3, 1)):
        vol = S.random_volume(shape, dtype, 7 + shape[2])
        for cell in CELLS:
            r.setVolume(vol, S.SPACING)
            nv, nt = r.extractIsosurface(ISO[dtype])
            assert (nt == 0) == (shape[2] == 1) and nt < 100
            simplify_and_compare(simplib, r, (shape, np.dtype(dtype).name), cell)
            if nt == 0:
                assert r.meshInfo() == dict(iso=ISO[dtype], vertices=0, triangles=0)


# ---------------------------------------------------------------- 2. content
@pytest.mark.parametrize("cell", CELLS)
def test_coincident_vertices_resolve_by_index(vra, simplib, handle, cell):
    r = handle
    r.setLayout(vra.renderer.LAYOUT_BRICKED)
    r.setVolume(S.ties_volume((40, 38, 36), 100, 5), S.SPACING)
    r.extractIsosurface(100)
    src, got = simplify_and_compare(simplib, r, "ties", cell)
    assert np.unique(src[0], axis=0).shape[0] < src[0].shape[0] - 1000          # the case exists


def simplify_a_key_case(vra, simplib, r, layout, name, cell, bits):
    make, iso, spacing = S.KEY_VOLUMES[name]
    r.setLayout(layout)
    r.setQuirks(vra.renderer.QUIRK_DEFAULT)
    r.setVolume(make(), spacing)
    nv, nt = r.extractIsosurface(iso)
    assert nt > 0
    S.assert_key_case(r.readMesh()[0], name, cell, bits)     # the widths, before the device is asked
    src, got = simplify_and_compare(simplib, r, ("keys", name), cell)
    assert 0 < got[2].shape[0] < nt
    if name == "ties":                                      # only coincident vertices share cells this small
        assert (nv, nt) == (162035, 327616) and (got[0].shape[0], got[2].shape[0]) == (99298, 220946)
    assert r.meshInfo() == dict(iso=iso, vertices=got[0].shape[0], triangles=got[2].shape[0])


@pytest.mark.parametrize("name,cell,bits", S.KEY_CASES, ids=S.KEY_CASE_IDS)
def test_keys_wider_than_32_bits_and_axes_without_bits(vra, simplib, handle, name, cell, bits):
    """the three cell indices are packed into one 64-bit key, each in the bits the extent needs: 36, 39, 57 and all 63 bits of it, three
    unequal widths, and no bits at all for z or for x.  The 63-bit cell is the largest quotient the call accepts."""
    simplify_a_key_case(vra, simplib, handle, vra.renderer.LAYOUT_BRICKED, name, cell, bits)


LINEAR_KEY_CASES = [S.KEY_CASE_IDS.index("ties, 63 bits"), S.KEY_CASE_IDS.index("flat x, 16 bits")]


@pytest.mark.parametrize("at", LINEAR_KEY_CASES, ids=[S.KEY_CASE_IDS[at] for at in LINEAR_KEY_CASES])
def test_wide_keys_on_the_linear_layout(vra, simplib, handle, at):
    simplify_a_key_case(vra, simplib, handle, vra.renderer.LAYOUT_LINEAR, *S.KEY_CASES[at])


def test_a_smoothed_volume_and_a_filtered_mesh(vra, oracle, simplib, handle):
    r = handle
    R = vra.renderer
    vol = oracle.gen_noise_ball((41, 39, 40), 2, 77)
    iso = (int(vol.min()) + int(vol.max())) // 2 - 1000
    r.setLayout(R.LAYOUT_BRICKED)
    r.setQuirks(R.QUIRK_DEFAULT)
    r.setVolume(vol, S.SPACING)
    try:
        r.smoothVolume(sigma_voxels=(1.0, 1.0, 1.0))
        assert r.extractIsosurface(iso)[1] > 0
        for cell in (1.5, 4.0):
            r.extractIsosurface(iso)
            simplify_and_compare(simplib, r, "smoothed", cell)
    finally:
        r.smoothVolume(sigma_voxels=0.0)
    n = r.labelComponents(iso)
    assert n >= 1
    labels = r.readLabels()
    try:
        assert r.selectComponents(0, 1) == 1
        for cell in (1.5, 4.0):
            nv, nt = r.extractComponents()
            assert 0 < nt
            simplify_and_compare(simplib, r, "largest component", cell)
            assert np.array_equal(r.readLabels(), labels) and r.componentsInfo()["selected"] == 1     # the labelling survives
        assert r.extractIsosurface(iso)[1] >= nt
    finally:
        r.freeComponents()


# ---------------------------------------------------------------- 3. repeat
def test_a_second_call_is_the_identity_and_a_larger_cell_simplifies_the_result(vra, simplib, handle):
    r = handle
    r.setLayout(vra.renderer.LAYOUT_BRICKED)
    r.setVolume(S.random_volume((40, 38, 36), np.uint8, 9), S.SPACING)
    r.extractIsosurface(128)
    src, first = simplify_and_compare(simplib, r, "repeat", 1.5)
    assert r.simplifyMesh(1.5) == (first[0].shape[0], first[2].shape[0])
    assert_same_mesh(r.readMesh(), first, "the same cell again")
    assert r.meshSimplification() == dict(cell=1.5, source_vertices=first[0].shape[0], source_triangles=first[2].shape[0])
    want, _ = simp_ref.simplify(simplib, first, 4.0)
    assert r.simplifyMesh(4.0) == (want[0].shape[0], want[2].shape[0])
    assert_same_mesh(r.readMesh(), want, "a larger cell on the result")
    assert 0 < want[2].shape[0] < first[2].shape[0] < src[2].shape[0]


# ---------------------------------------------------------------- 4. state
def frame(r):
    r.render()
    rgba = r.readPixels().copy()
    total, spp = r.countSamples(per_pixel=True)
    return rgba, spp.copy(), total


def test_simplification_leaves_the_renderer_alone(vra, oracle, simplib, handle):
    r = handle
    R = vra.renderer
    vol = oracle.gen_noise_ball((41, 39, 40), 2, 77)
    iso = (int(vol.min()) + int(vol.max())) // 2 - 1000
    r.setLayout(R.LAYOUT_BRICKED)
    r.setQuirks(R.QUIRK_DEFAULT)
    r.setVolume(vol)
    r.freeMesh()
    r.freeComponents()
    with pytest.raises(vra.VRError) as e:
        r.meshSimplification()
    assert e.value.code == R.VR_E_INVALID
    n = r.labelComponents(iso)
    labels = r.readLabels()
    before = frame(r)
    r.takeMessage()
    base = r.residentBytes()[2]
    nv, nt = r.extractIsosurface(iso)
    assert r.meshSimplification() == dict(cell=0.0, source_vertices=nv, source_triangles=nt)
    assert r.residentBytes()[2] == base + 24 * nv + 12 * nt
    state = (r.window, r.residentBytes()[:2], bits(r.getCameraBlock()).tolist(), r.smoothing)
    choice, kernel = r.last_launch_choice, r.last_kernel_name
    src, got = simplify_and_compare(simplib, r, "state", 2.0)
    nv2, nt2 = got[0].shape[0], got[2].shape[0]
    assert 0 < nt2 < nt and r.takeMessage() is None and r.simplifyMs() > 0.0
    assert r.meshInfo() == dict(iso=iso, vertices=nv2, triangles=nt2)
    assert r.residentBytes()[2] == base + 24 * nv2 + 12 * nt2               # no work array is left behind
    assert (r.last_launch_choice, r.last_kernel_name) == (choice, kernel)
    assert (r.window, r.residentBytes()[:2], bits(r.getCameraBlock()).tolist(), r.smoothing) == state
    assert np.array_equal(r.readLabels(), labels) and r.componentsInfo()["components"] == n
    after = frame(r)
    assert np.array_equal(bits(after[0]), bits(before[0])) and np.array_equal(after[1], before[1]) and after[2] == before[2]
    assert r.extractIsosurface(iso) == (nv, nt)
    assert r.meshSimplification() == dict(cell=0.0, source_vertices=nv, source_triangles=nt)
    assert_same_mesh(r.readMesh(), src, "a fresh extraction")
    r.freeMesh()
    r.freeComponents()
    assert r.residentBytes()[2] == base - 4 * vol.size


# ---------------------------------------------------------------- 5. errors
def test_refused_calls_leave_the_mesh_alone(vra, handle):
    r = handle
    R = vra.renderer
    r.setLayout(R.LAYOUT_BRICKED)
    r.setVolume(S.random_volume((13, 11, 6), np.uint8, 3), S.SPACING)
    nv, nt = r.extractIsosurface(128)
    mesh = r.readMesh()
    assert nt > 0
    r.takeMessage()
    for cell in (0.0, -1.0, float("nan"), float("inf"), 1e-40):
        with pytest.raises(vra.VRError) as e:
            r.simplifyMesh(cell)
        assert e.value.code == R.VR_E_INVALID and r.takeMessage() is None
        assert_same_mesh(r.readMesh(), mesh, f"cell {cell}")
    extent = float(mesh[0].max())
    assert extent >= 5.0
    with pytest.raises(vra.VRError) as e:
        r.simplifyMesh(extent / 2097152.0)                   # the largest coordinate's quotient is 2^21
    assert e.value.code == R.VR_E_INVALID
    message = r.takeMessage()
    assert message is not None and message[0] == "Error!"
    assert_same_mesh(r.readMesh(), mesh, "a quotient of 2^21")
    assert r.meshSimplification() == dict(cell=0.0, source_vertices=nv, source_triangles=nt)
    assert r.meshInfo() == dict(iso=128, vertices=nv, triangles=nt)
    r.freeMesh()
    for call in (lambda: r.simplifyMesh(1.0), r.meshSimplification):
        with pytest.raises(vra.VRError) as e:
            call()
        assert e.value.code == R.VR_E_INVALID


# ---------------------------------------------------------------- 6. files
def test_saved_files_carry_the_simplified_mesh(vra, simplib, handle, tmp_path):
    r = handle
    r.setLayout(vra.renderer.LAYOUT_BRICKED)
    r.setVolume(S.random_volume((13, 11, 6), np.uint16, 4), S.SPACING)
    full = r.extractIsosurface(30000)
    src, (pos, nrm, tri) = simplify_and_compare(simplib, r, "files", 1.5)
    nv, nt = pos.shape[0], tri.shape[0]
    assert 0 < nt < full[1]
    r.saveMesh(tmp_path / "s.ply", "ply")
    raw = (tmp_path / "s.ply").read_bytes()
    assert f"element vertex {nv}\n".encode() in raw and f"element face {nt}\n".encode() in raw
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    assert len(raw) == end + 24 * nv + 13 * nt
    verts = np.frombuffer(raw, dtype="<f4", count=6 * nv, offset=end).reshape(nv, 6)
    assert np.array_equal(verts[:, :3].view(np.uint32), pos.view(np.uint32)) and np.array_equal(verts[:, 3:].view(np.uint32), nrm.view(np.uint32))
    faces = np.frombuffer(raw, dtype=np.uint8, offset=end + 24 * nv).reshape(nt, 13)
    assert np.all(faces[:, 0] == 3) and np.array_equal(np.ascontiguousarray(faces[:, 1:]).view("<u4"), tri)
    r.saveMesh(tmp_path / "s.stl", "stl")
    raw = (tmp_path / "s.stl").read_bytes()
    assert len(raw) == 84 + 50 * nt and struct.unpack_from("<I", raw, 80)[0] == nt
    rec = np.frombuffer(raw, dtype=np.uint8, offset=84).reshape(nt, 50)
    corners = np.ascontiguousarray(rec[:, 12:48]).view("<f4").reshape(nt, 3, 3)
    assert np.array_equal(corners.view(np.uint32), pos[tri.astype(np.int64)].view(np.uint32))
