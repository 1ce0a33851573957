"""Mesh smoothing without a GPU: the C ABI's new entry points, what a host-only handle answers, and the CPU definition
(tests/mesh_smooth_ref/mesh_smooth_ref.c), which tests/test_mesh_smooth_gpu.py holds the kernels to -- against answers worked out by
hand, against an independent numpy statement of the definition bit for bit, against the consequences its step 8 promises, and
against what smoothing is for: a ball gets rounder and, with Taubin's mu, keeps its volume."""
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
simp_ref = _load("simplify_ref_binding", _HERE / "simplify_ref" / "binding.py")
smooth_ref = _load("mesh_smooth_ref_binding", _HERE / "mesh_smooth_ref" / "binding.py")
M = _load("mesh_checks", _HERE / "mesh_checks.py")
K = _load("mesh_smooth_cases", _HERE / "mesh_smooth_cases.py")


@pytest.fixture(scope="module")
def smoothlib(tmp_path_factory):
    return smooth_ref.build(tmp_path_factory.mktemp("mesh_smooth_ref"))


@pytest.fixture(scope="module")
def meshlib(tmp_path_factory):
    return mesh_ref.build(tmp_path_factory.mktemp("mesh_ref_mesh_smooth"))


@pytest.fixture(scope="module")
def simplib(tmp_path_factory):
    return simp_ref.build(tmp_path_factory.mktemp("simplify_ref_mesh_smooth"))


def same(got, want):
    problem = M.same_bits(got, want)
    assert not problem, problem


# ---------------------------------------------------------------- the C ABI
@pytest.mark.parametrize("name", ["vr_smooth_mesh", "vr_get_mesh_smoothing", "vr_get_mesh_smooth_ms"])
def test_library_exports_the_mesh_smoothing_entry_points(vra, name):
    assert name in vra.symbols_declared_in_header()
    assert hasattr(C.CDLL(str(vra.LIB_PATH)), name)


def test_host_only_handle_refuses_mesh_smoothing(vra):
    R = vra.renderer
    r = vra.RendererCore(-1)
    try:
        r.setup((64, 64))
        for args in ((10, 0.5, -0.53, True), (-1, 0.5, -0.53, True), (10, float("nan"), 0.0, False), (0, 0.5, 1.0, True)):
            with pytest.raises(vra.VRError) as e:           # the device is asked for before the arguments are looked at
                r.smoothMesh(*args)
            assert e.value.code == R.VR_E_NO_DEVICE
        with pytest.raises(vra.VRError) as e:
            r.meshSmoothing()
        assert e.value.code == R.VR_E_INVALID
        assert r.meshSmoothMs() == dict(build_ms=0.0, iterate_ms=0.0)       # 0 before the first call
        lib = vra.load_library()
        assert lib.vr_get_mesh_smooth_ms(r._h, None, None) == R.VR_E_INVALID
        one = C.c_float(-1.0)
        assert lib.vr_get_mesh_smooth_ms(r._h, C.byref(one), None) == R.VR_OK and one.value == 0.0
        one = C.c_float(-1.0)
        assert lib.vr_get_mesh_smooth_ms(r._h, None, C.byref(one)) == R.VR_OK and one.value == 0.0
        assert lib.vr_get_mesh_smoothing(r._h, None, None, None, None, None) == R.VR_E_INVALID      # no mesh
        assert lib.vr_smooth_mesh(None, 1, 0.5, -0.53, 1) == R.VR_E_INVALID
        assert lib.vr_get_mesh_smoothing(None, None, None, None, None, None) == R.VR_E_INVALID
    finally:
        r.close()


# ---------------------------------------------------------------- known answers
def mesh_of(pos, tri):
    pos = np.asarray(pos, dtype=np.float32).reshape(-1, 3)
    return pos, np.full_like(pos, 7.0), np.asarray(tri, dtype=np.uint32).reshape(-1, 3)


def tetrahedron():
    """closed, outward: every vertex has the other three as neighbours and every edge two triangles"""
    return mesh_of([[0, 0, 0], [4, 0, 0], [0, 8, 0], [0, 0, 16]], [[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])


def fan():
    """an open fan of six triangles about vertex 0 at height 3; the rim is a hexagon in the plane z = 0"""
    rim = [[4, 0, 0], [2, 4, 0], [-2, 4, 0], [-4, 0, 0], [-2, -4, 0], [2, -4, 0]]
    return mesh_of([[1, 1, 3]] + rim, [[0, 1 + q, 1 + (q + 1) % 6] for q in range(6)])


def test_a_closed_tetrahedron_moves_every_vertex_to_the_mean_of_the_others(smoothlib):
    src = tetrahedron()
    for fix in (True, False):
        (pos, nrm, tri), fixed = smooth_ref.smooth(smoothlib, src, 1, 1.0, 0.0, fix)
        assert not fixed.any()
        # the sums are of small integers and the quotients thirds: m is the rounded third, p + 1.0 * (m - p) within an ulp or two of it
        want = np.array([[4, 8, 16], [0, 8, 16], [4, 0, 16], [4, 8, 0]], dtype=np.float32) / np.float32(3.0)
        assert np.allclose(pos, want, rtol=3e-7, atol=0)
        assert tri is src[2] or np.array_equal(tri, src[2])
        same((pos, nrm, tri), K.numpy_smooth(src, 1, 1.0, 0.0, fix)[0])
        # the result is the tetrahedron mirrored in its centroid and shrunk to a third: the winding now faces inward
        centroid = src[0].mean(axis=0)
        assert np.all(np.einsum("ij,ij->i", nrm, pos - centroid) < 0.0)
        assert np.allclose(np.linalg.norm(nrm, axis=1), 1.0, atol=1e-6)


def test_an_open_fan_keeps_its_rim_and_centres_its_hub(smoothlib):
    src = fan()
    (pos, nrm, tri), fixed = smooth_ref.smooth(smoothlib, src, 1, 1.0, 0.0, True)
    assert fixed.tolist() == [False] + [True] * 6
    assert pos[0].tolist() == [0.0, 0.0, 0.0]                  # the rim's mean, exactly
    assert np.array_equal(pos[1:].view(np.uint32), src[0][1:].view(np.uint32))
    assert np.array_equal(nrm, np.tile(np.float32([0, 0, 1]), (7, 1)))      # flat now, counter-clockwise seen from +z
    same((pos, nrm, tri), K.numpy_smooth(src, 1, 1.0, 0.0, True)[0])
    assert K.consequences(src, (pos, nrm, tri), fixed) == ""
    (pos, nrm, tri), fixed = smooth_ref.smooth(smoothlib, src, 1, 1.0, 0.0, False)
    assert not fixed.any()
    assert pos[0].tolist() == [0.0, 0.0, 0.0]
    # a rim vertex has three neighbours: the hub and the two beside it
    assert np.allclose(pos[1], np.float32([1 + 2 + 2, 1 + 4 - 4, 3]) / np.float32(3.0), rtol=3e-7, atol=3e-7)
    assert not np.any(np.all(pos[1:] == src[0][1:], axis=1))
    same((pos, nrm, tri), K.numpy_smooth(src, 1, 1.0, 0.0, False)[0])


def test_a_vertex_no_triangle_references_stays_and_gets_no_normal(smoothlib):
    pos, nrm, tri = tetrahedron()
    pos = np.vstack([pos[:2], np.float32([[9, 9, 9]]), pos[2:]])           # vertex 2 is nobody's
    tri = np.where(tri >= 2, tri + 1, tri).astype(np.uint32)
    src = (pos, np.full_like(pos, 7.0), tri)
    for fix in (True, False):
        got, fixed = smooth_ref.smooth(smoothlib, src, 3, 0.5, -0.53, fix)
        assert got[0][2].tolist() == [9.0, 9.0, 9.0] and got[1][2].tolist() == [0.0, 0.0, 0.0] and not fixed.any()
        assert not np.any(np.all(got[0] == pos, axis=1)[[0, 1, 3, 4]])
        same(got, K.numpy_smooth(src, 3, 0.5, -0.53, fix)[0])
        assert K.consequences(src, got, fixed) == ""


def test_an_edge_shared_by_three_triangles_fixes_nothing_by_itself(smoothlib):
    """three triangles about the edge (0, 1): its multiplicity is 3, so it fixes neither end -- the six outer edges, each with one
    triangle, do.  Closing each wing with a second triangle over the same three vertices leaves no edge of multiplicity 1."""
    pos = [[0, 0, 0], [0, 0, 2], [3, 0, 1], [-1, 3, 1], [-1, -3, 1]]
    book = mesh_of(pos, [[0, 1, 2], [0, 1, 3], [0, 1, 4]])
    start, nbr, mult = K.graph(5, book[2])
    assert mult[(np.repeat(np.arange(5), np.diff(start)) == 0) & (nbr == 1)].tolist() == [3]
    got, fixed = smooth_ref.smooth(smoothlib, book, 1, 0.5, 0.0, True)
    assert fixed.all()                                        # through the outer edges
    doubled = mesh_of(pos, [[0, 1, 2], [0, 1, 3], [0, 1, 4], [1, 0, 2], [1, 0, 3], [1, 0, 4]])
    assert sorted(set(K.graph(5, doubled[2])[2].tolist())) == [2, 6]
    got, fixed = smooth_ref.smooth(smoothlib, doubled, 1, 0.5, 0.0, True)
    assert not fixed.any() and not np.any(np.all(got[0] == doubled[0], axis=1))
    same(got, K.numpy_smooth(doubled, 1, 0.5, 0.0, True)[0])


def test_a_triangle_with_a_repeated_corner_is_tolerated(smoothlib):
    src = mesh_of([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], [[0, 1, 2], [3, 3, 1], [2, 2, 2]])
    for fix in (True, False):
        got, fixed = smooth_ref.smooth(smoothlib, src, 2, 0.5, -0.53, fix)
        want, want_fixed = K.numpy_smooth(src, 2, 0.5, -0.53, fix)
        same(got, want)
        assert np.array_equal(fixed, want_fixed)


@pytest.mark.parametrize("args", [(-1, 0.5, -0.53), (1001, 0.5, -0.53), (1, 0.0, -0.53), (1, 1.5, -0.53), (1, float("nan"), 0.0),
                                  (1, float("inf"), 0.0), (1, 0.5, 0.1), (1, 0.5, -2.5), (1, 0.5, float("nan")), (1, 0.5, float("-inf"))])
def test_parameters_outside_their_ranges_are_refused(smoothlib, args):
    with pytest.raises(smooth_ref.SmoothError) as e:
        smooth_ref.smooth(smoothlib, tetrahedron(), *args, True)
    assert e.value.code == smooth_ref.BAD_PARAMETER


def test_the_ends_of_the_ranges_are_accepted(smoothlib):
    src = tetrahedron()
    for args in ((1000, 0.5, -0.53), (1, 1.0, -2.0), (1, 1e-30, -1e-30), (1, 0.5, -0.0)):
        got, _ = smooth_ref.smooth(smoothlib, src, *args, True)
        same(got, K.numpy_smooth(src, *args, True)[0])
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32))
    got, fixed = smooth_ref.smooth(smoothlib, empty, 10)
    assert got[0].shape == (0, 3) and got[1].shape == (0, 3) and got[2].shape == (0, 3) and fixed.size == 0


# ---------------------------------------------------------------- against the numpy statement, and the consequences
_MESHES = {}


def source_mesh(meshlib, simplib, name):
    """the meshes that are smoothed, extracted once by the extraction's CPU definition and left unchanged"""
    if name not in _MESHES:
        if name == "5x3x2":
            mesh = mesh_ref.extract(meshlib, K.random_volume((5, 3, 2), np.uint8, 9), 128.0, K.SPACING)
        elif name == "13x11x6":
            mesh = mesh_ref.extract(meshlib, K.random_volume((13, 11, 6), np.uint8, 30), 128.0, K.SPACING)
        elif name == "ties":
            mesh = mesh_ref.extract(meshlib, K.ties_volume((40, 38, 36), 100, 5), 100.0, K.SPACING)
        elif name == "ball":
            mesh = mesh_ref.extract(meshlib, K.ball_volume(), 128.0)
        elif name == "cut ball":
            mesh = mesh_ref.extract(meshlib, K.cut_ball_volume(), 128.0)
        elif name.startswith("13x11x6 simplified at "):
            mesh, _ = simp_ref.simplify(simplib, source_mesh(meshlib, simplib, "13x11x6"), float(name.rsplit(" ", 1)[1]))
        else:
            raise KeyError(name)
        for a in mesh:
            a.setflags(write=False)
        _MESHES[name] = mesh
    return _MESHES[name]


NAMES = ["5x3x2", "13x11x6", "ties", "ball", "cut ball", "13x11x6 simplified at 0.3", "13x11x6 simplified at 1.5"]


@pytest.mark.parametrize("name", NAMES)
def test_the_restatement_is_the_numpy_statement_and_has_the_consequences(smoothlib, meshlib, simplib, name):
    src = source_mesh(meshlib, simplib, name)
    assert src[2].shape[0] > 0
    big = src[2].shape[0] > 100000
    for args in ((3, 0.5, -0.53, True), (3, 0.5, -0.53, False)) + (() if big else ((2, 1.0, -2.0, True), (4, 0.25, 0.0, True))):
        got, fixed = smooth_ref.smooth(smoothlib, src, *args)
        want, want_fixed = K.numpy_smooth(src, *args)
        same(got, want)
        assert np.array_equal(fixed, want_fixed) and np.array_equal(fixed, K.fixed_vertices(src[0].shape[0], src[2], args[3]))
        assert K.consequences(src, got, fixed) == ""
        assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1]))
        if not args[3]:
            assert not fixed.any()


def test_the_case_meshes_are_what_their_names_say(meshlib, simplib):
    ties = source_mesh(meshlib, simplib, "ties")
    assert np.unique(ties[0], axis=0).shape[0] < ties[0].shape[0] - 1000     # coincident vertices in droves
    got, _ = K.numpy_smooth(ties, 1)
    assert np.any(np.all(got[1] == 0.0, axis=1))                             # ... and normals that are zero
    assert K.fixed_vertices(ties[0].shape[0], ties[2], True).any()           # the surface meets the volume's boundary
    fine = source_mesh(meshlib, simplib, "13x11x6 simplified at 0.3")
    coarse = source_mesh(meshlib, simplib, "13x11x6 simplified at 1.5")
    assert K.degree_and_multiplicity(fine[0].shape[0], fine[2])[1] > 2       # edges with more than two triangles
    assert 0 < coarse[2].shape[0] < fine[2].shape[0] < source_mesh(meshlib, simplib, "13x11x6")[2].shape[0]


@pytest.mark.parametrize("name", ["13x11x6", "cut ball", "13x11x6 simplified at 1.5"])
def test_calls_accumulate_and_no_iteration_is_the_identity(smoothlib, meshlib, simplib, name):
    src = source_mesh(meshlib, simplib, name)
    for fix in (True, False):
        whole, fixed = smooth_ref.smooth(smoothlib, src, 5, 0.5, -0.53, fix)
        first, fixed_first = smooth_ref.smooth(smoothlib, src, 2, 0.5, -0.53, fix)
        second, fixed_second = smooth_ref.smooth(smoothlib, first, 3, 0.5, -0.53, fix)
        same(second, whole)
        assert np.array_equal(fixed, fixed_first) and np.array_equal(fixed, fixed_second)
        assert np.array_equal(whole[0][fixed].view(np.uint32), src[0][fixed].view(np.uint32))      # fixed rows keep their bits
        assert np.array_equal(whole[2], src[2])
    same(smooth_ref.smooth(smoothlib, src, 0)[0], src)
    same(K.numpy_smooth(src, 0)[0], src)


# ---------------------------------------------------------------- what it is for
def radius_deviation(pos):
    return float(np.linalg.norm(pos.astype(np.float64) - 31.5, axis=1).std())


def test_the_ball_gets_rounder_and_taubin_keeps_its_volume(smoothlib, meshlib, simplib):
    src = source_mesh(meshlib, simplib, "ball")
    assert (src[0].shape[0], src[2].shape[0]) == (32714, 65424)
    assert M.closed_and_oriented(src[2]) == ""
    volume = M.signed_volume(src[0], src[2])
    got, fixed = smooth_ref.smooth(smoothlib, src, **K.DEFAULTS)
    assert int(fixed.sum()) == 0
    before, after = radius_deviation(src[0]), radius_deviation(got[0])
    taubin = M.signed_volume(got[0], got[2])
    laplace = M.signed_volume(*smooth_ref.smooth(smoothlib, src, 10, 0.5, 0.0)[0][::2])
    print(f"radius deviation {before:.4f} -> {after:.4f}; volume {volume:.2f}, Taubin {taubin:.2f}, Laplacian {laplace:.2f}")
    assert after < before
    assert abs(taubin - volume) < 0.001 * volume
    assert volume - laplace > 0.003 * volume
    radial = got[0].astype(np.float64) - 31.5
    radial /= np.linalg.norm(radial, axis=1)[:, None]
    assert np.einsum("ij,ij->i", got[1].astype(np.float64), radial).min() >= 0.99
    assert np.einsum("ij,ij->i", got[1].astype(np.float64), src[1].astype(np.float64)).min() >= 0.99


def test_the_cut_ball_keeps_its_cut(smoothlib, meshlib, simplib):
    src = source_mesh(meshlib, simplib, "cut ball")
    got, fixed = smooth_ref.smooth(smoothlib, src, **K.DEFAULTS)
    assert int(fixed.sum()) == 314
    assert np.all(src[0][fixed, 0] == 39.0)
    assert np.array_equal(got[0][fixed].view(np.uint32), src[0][fixed].view(np.uint32))
    assert np.any(got[0][~fixed] != src[0][~fixed], axis=1).mean() > 0.99
    assert float(got[0][:, 0].max()) == 39.0                   # nothing crosses the plane of the cut
