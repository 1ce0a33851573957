"""vr_smooth_mesh on the device against its CPU definition (tests/mesh_smooth_ref/mesh_smooth_ref.c), bit for bit as arrays: the
mesh the device holds is read back, smoothed by the restatement and compared with what the device made of it -- both voxel types,
both layouts, a handful of triangles, the empty mesh and a million vertices, coincident vertices, open and closed surfaces,
simplified meshes with vertices of degree 25 and edges of seven triangles, filtered and smoothed-volume meshes, the ends of the
parameter ranges, repeated calls, what the call does to the handle's state, what it refuses, and the file written from its result."""
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


smooth_ref = _load("mesh_smooth_ref_binding", _HERE / "mesh_smooth_ref" / "binding.py")
M = _load("mesh_checks", _HERE / "mesh_checks.py")
K = _load("mesh_smooth_cases", _HERE / "mesh_smooth_cases.py")

ISO = {np.uint8: 128, np.uint16: 30000}
LAYOUTS = pytest.mark.parametrize("layout", [0, 1], ids=["linear", "bricked"])
DTYPES = pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
DEFAULTS = (10, 0.5, -0.53, True)


@pytest.fixture(scope="module")
def smoothlib(tmp_path_factory):
    return smooth_ref.build(tmp_path_factory.mktemp("mesh_smooth_ref_gpu"))


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


def source_and_reference(smoothlib, r, key, args):
    """the device's resident (unsmoothed) mesh and the restatement's smoothing of it.  Both layouts extract the same mesh
    (tests/test_mesh_gpu.py), so it is read and smoothed on the CPU once per (key, args) and the later reader only compares."""
    src = r.readMesh()
    if key not in _SOURCE:
        for a in src:
            a.setflags(write=False)
        _SOURCE[key] = src
    else:
        assert_same_mesh(src, _SOURCE[key], f"{key}: the mesh to smooth")
    if (key, args) not in _REF:
        want, fixed = smooth_ref.smooth(smoothlib, _SOURCE[key], *args)
        for a in want:
            a.setflags(write=False)
        _REF[(key, args)] = want, int(fixed.sum())
    return _SOURCE[key], _REF[(key, args)]


def smooth_and_compare(smoothlib, r, key, args=DEFAULTS):
    src, (want, n_fixed) = source_and_reference(smoothlib, r, key, args)
    assert r.smoothMesh(*args) == n_fixed, f"{key}, {args}: fixed vertices"
    got = r.readMesh()
    assert_same_mesh(got, want, f"{key}, {args}")
    assert r.meshSmoothing() == dict(iterations=args[0], lam=float(np.float32(args[1])), mu=float(np.float32(args[2])), fix_boundary=bool(args[3]),
                                     fixed_vertices=n_fixed)
    return src, got, n_fixed


# ---------------------------------------------------------------- 1. shapes and types
@DTYPES
@LAYOUTS
@pytest.mark.parametrize("shape", [(13, 11, 6), (70, 66, 68)], ids=lambda s: "x".join(map(str, s)))
def test_smoothing_matches_the_reference(vra, smoothlib, handle, shape, layout, dtype):
    r = handle
    seed = sum(shape) + np.dtype(dtype).itemsize
    r.setLayout(layout)
    r.setQuirks(vra.renderer.QUIRK_DEFAULT)
    r.setVolume(K.random_volume(shape, dtype, seed), K.SPACING)
    nv, nt = r.extractIsosurface(ISO[dtype])
    big = shape == (70, 66, 68)
    if big:
        assert nv > 4096 * 256 and 6 * nt > 6000000          # the grid's second row; sorts and scans over many blocks
    src, got, n_fixed = smooth_and_compare(smoothlib, r, (shape, np.dtype(dtype).name), (3,) + DEFAULTS[1:] if big else DEFAULTS)
    assert 0 < n_fixed < nv
    assert r.meshInfo() == dict(iso=ISO[dtype], vertices=nv, triangles=nt)
    assert K.consequences(src, got, K.fixed_vertices(nv, src[2], True)) == ""


@DTYPES
@LAYOUTS
def test_a_handful_of_triangles_and_the_empty_mesh(vra, smoothlib, handle, layout, dtype):
    r = handle
    r.setLayout(layout)
    r.setQuirks(vra.renderer.QUIRK_DEFAULT)
    for shape in ((5, 3, 2), (5, 3, 1)):
        vol = K.random_volume(shape, dtype, 7 + shape[2])
        for args in (DEFAULTS, (1, 0.5, -0.53, False), (1000, 0.5, -0.53, True), (1000, 0.5, -0.53, False)):
            r.setVolume(vol, K.SPACING)
            nv, nt = r.extractIsosurface(ISO[dtype])
            assert (nt == 0) == (shape[2] == 1) and nt < 100
            smooth_and_compare(smoothlib, r, (shape, np.dtype(dtype).name), args)
            assert r.meshInfo() == dict(iso=ISO[dtype], vertices=nv, triangles=nt)
            if nt == 0:
                assert r.meshSmoothMs() == dict(build_ms=0.0, iterate_ms=0.0)


# ---------------------------------------------------------------- 2. graphs
def test_coincident_vertices_are_different_vertices(vra, smoothlib, handle):
    r = handle
    r.setLayout(vra.renderer.LAYOUT_BRICKED)
    r.setVolume(K.ties_volume((40, 38, 36), 100, 5), K.SPACING)
    r.extractIsosurface(100)
    src, got, n_fixed = smooth_and_compare(smoothlib, r, "ties")
    assert np.unique(src[0], axis=0).shape[0] < src[0].shape[0] - 1000          # the case exists
    r.extractIsosurface(100)
    src, got, n_fixed = smooth_and_compare(smoothlib, r, "ties", (1,) + DEFAULTS[1:])
    assert np.any(np.all(got[1] == 0.0, axis=1))                                # ... and so do normals that are zero


def test_a_closed_ball_fixes_nothing_and_a_cut_ball_its_cut(vra, smoothlib, handle):
    r = handle
    r.setLayout(vra.renderer.LAYOUT_BRICKED)
    r.setVolume(K.ball_volume())
    assert r.extractIsosurface(128) == (32714, 65424)
    src, got, n_fixed = smooth_and_compare(smoothlib, r, "ball")
    assert n_fixed == 0 and M.closed_and_oriented(got[2]) == ""
    assert abs(M.signed_volume(got[0], got[2]) - M.signed_volume(src[0], src[2])) < 0.001 * M.signed_volume(src[0], src[2])
    r.setVolume(K.cut_ball_volume())
    r.extractIsosurface(128)
    src, got, n_fixed = smooth_and_compare(smoothlib, r, "cut ball")
    fixed = K.fixed_vertices(src[0].shape[0], src[2], True)
    assert n_fixed == 314 == int(fixed.sum()) and np.all(src[0][fixed, 0] == 39.0)
    assert np.array_equal(bits(got[0][fixed]), bits(src[0][fixed]))


@pytest.mark.parametrize("cell", [0.3, 1.5])
def test_simplified_meshes_with_high_degrees_and_edges_of_many_triangles(vra, smoothlib, handle, cell):
    r = handle
    r.setLayout(vra.renderer.LAYOUT_BRICKED)
    r.setQuirks(vra.renderer.QUIRK_DEFAULT)
    r.setVolume(K.random_volume((70, 66, 68), np.uint8, 70 + 66 + 68 + 1), K.SPACING)
    r.extractIsosurface(128)
    nv, nt = r.simplifyMesh(cell)
    simplification = r.meshSimplification()
    src, got, n_fixed = smooth_and_compare(smoothlib, r, ("simplified", cell), (3,) + DEFAULTS[1:])
    degree, multiplicity = K.degree_and_multiplicity(nv, src[2])
    if cell == 0.3:
        assert degree >= 20 and multiplicity >= 4, (degree, multiplicity)
    else:
        assert 2 * n_fixed > nv                              # more than half the vertices do not move
    assert r.meshSimplification() == simplification and r.meshInfo() == dict(iso=128, vertices=nv, triangles=nt)


def test_a_filtered_mesh_and_the_mesh_of_a_smoothed_volume(vra, oracle, smoothlib, handle):
    r = handle
    R = vra.renderer
    vol = oracle.gen_noise_ball((41, 39, 40), 2, 77)
    iso = (int(vol.min()) + int(vol.max())) // 2 - 1000
    r.setLayout(R.LAYOUT_BRICKED)
    r.setQuirks(R.QUIRK_DEFAULT)
    r.setVolume(vol, K.SPACING)
    try:
        r.smoothVolume(sigma_voxels=(1.0, 1.0, 1.0))
        assert r.extractIsosurface(iso)[1] > 0
        smooth_and_compare(smoothlib, r, "smoothed volume")
    finally:
        r.smoothVolume(sigma_voxels=0.0)
    n = r.labelComponents(iso)
    assert n >= 1
    labels = r.readLabels()
    try:
        assert r.selectComponents(0, 1) == 1
        nv, nt = r.extractComponents()
        assert 0 < nt
        smooth_and_compare(smoothlib, r, "largest component")
        assert np.array_equal(r.readLabels(), labels) and r.componentsInfo()["selected"] == 1     # the labelling survives
    finally:
        r.freeComponents()


# ---------------------------------------------------------------- 3. parameters
@pytest.mark.parametrize("args", [(1, 1.0, -0.53, True), (2, 1.0, -2.0, True), (3, 0.5, 0.0, True), (3, 0.5, -0.0, False), (1, 0.5, -2.0, False),
                                  (1, 0.5, -0.53, True), (2, 2.0 ** -20, -(2.0 ** -20), False)], ids=str)
def test_the_ends_of_the_parameter_ranges(vra, smoothlib, handle, args):
    r = handle
    r.setLayout(vra.renderer.LAYOUT_BRICKED)
    r.setQuirks(vra.renderer.QUIRK_DEFAULT)
    r.setVolume(K.random_volume((13, 11, 6), np.uint8, 3), K.SPACING)
    r.extractIsosurface(128)
    src, got, n_fixed = smooth_and_compare(smoothlib, r, "parameters", args)
    assert (n_fixed == 0) == (not args[3])
    assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1]))


# ---------------------------------------------------------------- 4. repeat
def test_calls_accumulate_and_no_iteration_changes_nothing(vra, smoothlib, handle):
    r = handle
    r.setLayout(vra.renderer.LAYOUT_BRICKED)
    r.setVolume(K.random_volume((40, 38, 36), np.uint8, 9), K.SPACING)
    r.extractIsosurface(128)
    src, whole, n_fixed = smooth_and_compare(smoothlib, r, "repeat", (5, 0.5, -0.53, True))
    r.extractIsosurface(128)
    assert r.smoothMesh(0) == 0
    assert_same_mesh(r.readMesh(), src, "no iteration")       # the gradient normals too
    assert r.meshSmoothing() == dict(iterations=0, lam=0.5, mu=float(np.float32(-0.53)), fix_boundary=True, fixed_vertices=0)
    assert r.meshSmoothMs() == dict(build_ms=0.0, iterate_ms=0.0)
    assert r.smoothMesh(2, 0.5, -0.53, True) == n_fixed
    ms = r.meshSmoothMs()
    assert ms["build_ms"] > 0.0 and ms["iterate_ms"] > 0.0
    assert r.smoothMesh(3, 0.5, -0.53, True) == n_fixed
    assert_same_mesh(r.readMesh(), whole, "2 then 3 iterations against 5")
    assert r.meshSmoothing()["iterations"] == 3
    smoothed = r.readMesh()
    assert r.smoothMesh(0, 1.0, 0.0, False) == 0
    assert_same_mesh(r.readMesh(), smoothed, "no iteration on a smoothed mesh")       # its recomputed normals stay
    assert r.meshSmoothMs() == dict(build_ms=0.0, iterate_ms=0.0)


# ---------------------------------------------------------------- 5. state
def frame(r):
    r.render()
    rgba = r.readPixels().copy()
    total, spp = r.countSamples(per_pixel=True)
    return rgba, spp.copy(), total


def test_smoothing_leaves_the_renderer_alone(vra, oracle, smoothlib, handle):
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
        r.meshSmoothing()
    assert e.value.code == R.VR_E_INVALID
    n = r.labelComponents(iso)
    labels = r.readLabels()
    before = frame(r)
    r.takeMessage()
    base = r.residentBytes()[2]
    nv, nt = r.extractIsosurface(iso)
    unsmoothed = dict(iterations=0, lam=0.0, mu=0.0, fix_boundary=False, fixed_vertices=0)
    assert r.meshSmoothing() == unsmoothed
    state = (r.window, r.residentBytes()[:2], bits(r.getCameraBlock()).tolist(), r.smoothing)
    choice, kernel = r.last_launch_choice, r.last_kernel_name
    info, simplification = r.meshInfo(), r.meshSimplification()
    src, got, n_fixed = smooth_and_compare(smoothlib, r, "state")
    assert r.takeMessage() is None
    ms = r.meshSmoothMs()
    assert ms["build_ms"] > 0.0 and ms["iterate_ms"] > 0.0
    assert r.meshInfo() == info and r.meshSimplification() == simplification
    assert r.residentBytes()[2] == base + 24 * nv + 12 * nt                 # no work array is left behind
    assert (r.last_launch_choice, r.last_kernel_name) == (choice, kernel)
    assert (r.window, r.residentBytes()[:2], bits(r.getCameraBlock()).tolist(), r.smoothing) == state
    assert np.array_equal(r.readLabels(), labels) and r.componentsInfo()["components"] == n
    after = frame(r)
    assert np.array_equal(bits(after[0]), bits(before[0])) and np.array_equal(after[1], before[1]) and after[2] == before[2]
    # a new mesh is unsmoothed: after an extraction, and after a simplification
    assert r.extractIsosurface(iso) == (nv, nt)
    assert r.meshSmoothing() == unsmoothed
    assert_same_mesh(r.readMesh(), src, "a fresh extraction")
    r.smoothMesh(1)
    assert r.meshSmoothing()["iterations"] == 1
    r.extractIsosurface(iso)
    r.simplifyMesh(2.0)
    r.smoothMesh(1)
    assert r.meshSmoothing()["iterations"] == 1 and r.meshSimplification()["cell"] == 2.0
    r.extractIsosurface(iso)
    r.smoothMesh(2, 0.25, 0.0, False)                         # (no mu step: every coordinate stays a mean of coordinates >= 0)
    assert r.meshSmoothing() == dict(iterations=2, lam=0.25, mu=0.0, fix_boundary=False, fixed_vertices=0)
    r.simplifyMesh(2.0)
    assert r.meshSmoothing() == unsmoothed
    r.freeMesh()
    with pytest.raises(vra.VRError) as e:
        r.meshSmoothing()
    assert e.value.code == R.VR_E_INVALID
    r.freeComponents()
    assert r.residentBytes()[2] == base - 4 * vol.size


# ---------------------------------------------------------------- 6. errors
def test_refused_calls_leave_the_mesh_alone(vra, handle):
    r = handle
    R = vra.renderer
    r.setLayout(R.LAYOUT_BRICKED)
    r.setVolume(K.random_volume((13, 11, 6), np.uint8, 3), K.SPACING)
    nv, nt = r.extractIsosurface(128)
    assert nt > 0
    r.smoothMesh(1, 0.5, -0.53, True)
    mesh, smoothing = r.readMesh(), r.meshSmoothing()
    r.takeMessage()
    nan, inf = float("nan"), float("inf")
    for args in ((-1, 0.5, -0.53), (1001, 0.5, -0.53), (1, 0.0, -0.53), (1, -0.5, -0.53), (1, 1.0000001, -0.53), (1, nan, -0.53), (1, inf, -0.53),
                 (1, 0.5, 1e-30), (1, 0.5, -2.000001), (1, 0.5, nan), (1, 0.5, -inf), (0, 0.5, 0.5), (0, 2.0, 0.0)):
        with pytest.raises(vra.VRError) as e:
            r.smoothMesh(*args, True)
        assert e.value.code == R.VR_E_INVALID and r.takeMessage() is None, args
        assert_same_mesh(r.readMesh(), mesh, f"{args}")
        assert r.meshSmoothing() == smoothing and r.meshInfo() == dict(iso=128, vertices=nv, triangles=nt)
    r.freeMesh()
    for call in (lambda: r.smoothMesh(1), lambda: r.smoothMesh(0), r.meshSmoothing):
        with pytest.raises(vra.VRError) as e:
            call()
        assert e.value.code == R.VR_E_INVALID


def test_simplification_refuses_a_mesh_that_smoothing_pushed_below_zero(vra, smoothlib, handle):
    """the documented order is simplify, then smooth: a mu < 0 step can push a coordinate below 0 near the origin, and
    vr_simplify_mesh's step 2 refuses such a mesh"""
    r = handle
    R = vra.renderer
    r.setLayout(R.LAYOUT_BRICKED)
    r.setVolume(K.random_volume((13, 11, 6), np.uint8, 3), K.SPACING)
    r.extractIsosurface(128)
    src, got, n_fixed = smooth_and_compare(smoothlib, r, "parameters", (10, 0.5, -0.53, False))
    assert float(got[0].min()) < 0.0 <= float(src[0].min())                 # the case exists
    smoothing = r.meshSmoothing()
    r.takeMessage()
    with pytest.raises(vra.VRError) as e:
        r.simplifyMesh(1.5)
    assert e.value.code == R.VR_E_INVALID and r.takeMessage() is not None
    assert_same_mesh(r.readMesh(), got, "the refused simplification")
    assert r.meshSmoothing() == smoothing and r.meshSimplification()["cell"] == 0.0
    # the other way round works
    r.extractIsosurface(128)
    r.simplifyMesh(1.5)
    smooth_and_compare(smoothlib, r, "simplified first", (10, 0.5, -0.53, False))


# ---------------------------------------------------------------- 7. files
def test_a_saved_ply_carries_the_smoothed_arrays(vra, smoothlib, handle, tmp_path):
    r = handle
    r.setLayout(vra.renderer.LAYOUT_BRICKED)
    r.setVolume(K.random_volume((13, 11, 6), np.uint16, 4), K.SPACING)
    r.extractIsosurface(30000)
    src, (pos, nrm, tri), n_fixed = smooth_and_compare(smoothlib, r, "files")
    nv, nt = pos.shape[0], tri.shape[0]
    assert not np.array_equal(bits(pos), bits(src[0])) and not np.array_equal(bits(nrm), bits(src[1]))
    r.saveMesh(tmp_path / "s.ply", "ply")
    raw = (tmp_path / "s.ply").read_bytes()
    assert f"element vertex {nv}\n".encode() in raw and f"element face {nt}\n".encode() in raw
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    assert len(raw) == end + 24 * nv + 13 * nt
    verts = np.frombuffer(raw, dtype="<f4", count=6 * nv, offset=end).reshape(nv, 6)
    assert np.array_equal(verts[:, :3].view(np.uint32), pos.view(np.uint32)) and np.array_equal(verts[:, 3:].view(np.uint32), nrm.view(np.uint32))
    faces = np.frombuffer(raw, dtype=np.uint8, offset=end + 24 * nv).reshape(nt, 13)
    assert np.all(faces[:, 0] == 3) and np.array_equal(np.ascontiguousarray(faces[:, 1:]).view("<u4"), tri)
