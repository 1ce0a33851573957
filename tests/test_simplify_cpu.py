"""Mesh simplification without a GPU: the C ABI's new entry points, what a host-only handle answers, and the CPU definition
(tests/simplify_ref/simplify_ref.c), which tests/test_simplify_gpu.py holds the kernels to -- against answers worked out by hand,
against an independent numpy statement of the definition bit for bit, and against the consequences its step 6 promises."""
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
M = _load("mesh_checks", _HERE / "mesh_checks.py")
S = _load("simplify_cases", _HERE / "simplify_cases.py")


@pytest.fixture(scope="module")
def simplib(tmp_path_factory):
    return simp_ref.build(tmp_path_factory.mktemp("simplify_ref"))


@pytest.fixture(scope="module")
def meshlib(tmp_path_factory):
    return mesh_ref.build(tmp_path_factory.mktemp("mesh_ref_simplify"))


# ---------------------------------------------------------------- the C ABI
@pytest.mark.parametrize("name", ["vr_simplify_mesh", "vr_get_mesh_simplification", "vr_get_simplify_ms"])
def test_library_exports_the_simplification_entry_points(vra, name):
    assert name in vra.symbols_declared_in_header()
    assert hasattr(C.CDLL(str(vra.LIB_PATH)), name)


def test_host_only_handle_refuses_simplification(vra):
    R = vra.renderer
    r = vra.RendererCore(-1)
    try:
        r.setup((64, 64))
        for cell in (1.0, 0.0, float("nan")):               # the device is asked for before the cell is looked at
            with pytest.raises(vra.VRError) as e:
                r.simplifyMesh(cell)
            assert e.value.code == R.VR_E_NO_DEVICE
        for call in (r.meshSimplification, r.meshInfo):
            with pytest.raises(vra.VRError) as e:
                call()
            assert e.value.code == R.VR_E_INVALID
        assert r.simplifyMs() == 0.0                          # 0 before the first call
        lib = vra.load_library()
        assert lib.vr_get_simplify_ms(r._h, None) == R.VR_E_INVALID
        assert lib.vr_simplify_mesh(None, 1.0, None, None) == R.VR_E_INVALID
    finally:
        r.close()


# ---------------------------------------------------------------- known answers
def hand_mesh():
    """cell 1.  Cell A = (0,0,0) holds v0 (far) and v1 (at the centre): v1 wins although its index is higher.  Cell B = (1,0,0)
    holds v2 and v3 at the same distance either side of the centre: the lower index wins.  v4, v5, v7 are alone in their cells.
    v6 is alone in its cell and only a collapsing triangle references it."""
    pos = np.array([[0.875, 0.5, 0.5], [0.5, 0.5, 0.5], [1.25, 0.5, 0.5], [1.75, 0.5, 0.5], [0.5, 1.5, 0.5], [0.5, 0.5, 1.5],
                    [2.5, 2.5, 2.5], [1.5, 1.5, 0.5]], dtype=np.float32)
    nrm = np.arange(24, dtype=np.float32).reshape(8, 3)       # any bits: they travel with their vertex
    tri = np.array([[0, 2, 4],      # -> (1, 2, 4): kept
                    [0, 1, 6],      # -> (1, 1, 6): collapses
                    [1, 3, 4],      # -> (1, 2, 4): the set of triangle 0, same orientation
                    [4, 3, 0],      # -> (4, 2, 1): the set of triangle 0, opposite orientation
                    [3, 1, 5],      # -> (2, 1, 5): kept
                    [5, 0, 2],      # -> (5, 1, 2): the set of triangle 4, opposite orientation
                    [2, 7, 4]],     # kept as it is
                   dtype=np.uint32)
    return pos, nrm, tri


def test_every_rule_on_a_mesh_checked_by_eye(simplib):
    src = hand_mesh()
    (pos, nrm, tri), rows = simp_ref.simplify(simplib, src, 1.0)
    assert rows.tolist() == [1, 2, 4, 5, 7]
    assert tri.tolist() == [[0, 1, 2], [1, 0, 3], [1, 4, 2]]
    assert np.array_equal(pos, src[0][rows]) and np.array_equal(nrm, src[1][rows])
    assert S.consequences(src, (pos, nrm, tri), rows, 1.0) == ""
    want, want_rows = S.numpy_simplify(src, 1.0)
    assert M.same_bits((pos, nrm, tri), want) == "" and np.array_equal(rows, want_rows)


def test_a_cell_larger_than_the_extent_and_the_empty_mesh(simplib):
    src = hand_mesh()
    (pos, nrm, tri), rows = simp_ref.simplify(simplib, src, 3.0)
    assert pos.shape == (0, 3) and nrm.shape == (0, 3) and tri.shape == (0, 3) and rows.size == 0
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32))
    (pos, nrm, tri), rows = simp_ref.simplify(simplib, empty, 1.0)
    assert pos.shape == (0, 3) and tri.shape == (0, 3)
    (pos, nrm, tri), rows = simp_ref.simplify(simplib, (src[0], src[1], src[2][:0]), 1.0)     # vertices without a triangle
    assert pos.shape == (0, 3) and tri.shape == (0, 3)


@pytest.mark.parametrize("cell", [0.0, -1.0, float("nan"), float("inf"), 1e-40])
def test_a_cell_that_is_no_positive_normal_number_is_refused(simplib, cell):
    with pytest.raises(simp_ref.SimplifyError) as e:
        simp_ref.simplify(simplib, hand_mesh(), cell)
    assert e.value.code == simp_ref.BAD_CELL


def test_a_quotient_of_2_to_the_21_is_refused_and_the_one_below_it_accepted(simplib):
    below = float(np.nextafter(np.float32(2097152.0), np.float32(0.0)))
    nrm = np.zeros((3, 3), dtype=np.float32)
    tri = np.array([[0, 1, 2]], dtype=np.uint32)
    for axis in range(3):
        pos = np.zeros((3, 3), dtype=np.float32)
        pos[1, axis] = 5.0
        pos[2, axis] = below
        got, rows = simp_ref.simplify(simplib, (pos, nrm, tri), 1.0)
        assert M.same_bits(got, (pos, nrm, tri)) == "" and rows.tolist() == [0, 1, 2]
        assert M.same_bits(S.numpy_simplify((pos, nrm, tri), 1.0)[0], got) == ""
        pos[2, axis] = 2097152.0
        with pytest.raises(simp_ref.SimplifyError) as e:
            simp_ref.simplify(simplib, (pos, nrm, tri), 1.0)
        assert e.value.code == simp_ref.OVERFLOW
        with pytest.raises(OverflowError):
            S.numpy_simplify((pos, nrm, tri), 1.0)
        got, _ = simp_ref.simplify(simplib, (pos, nrm, tri), 2.0)          # the same mesh on larger cells fits
        assert got[2].shape[0] == 1
    # the quotient counts, not the coordinate
    pos = np.array([[0, 0, 0], [0.25, 0, 0], [0.5, 0, 0]], dtype=np.float32)
    with pytest.raises(simp_ref.SimplifyError):
        simp_ref.simplify(simplib, (pos, nrm, tri), 0.5 / 2097152.0)


# ---------------------------------------------------------------- against the numpy statement, and the consequences
_MESHES = {}


def source_mesh(meshlib, name):
    """the meshes that are simplified, extracted once by the extraction's CPU definition and left unchanged"""
    if name not in _MESHES:
        if name == "random_u8":
            mesh = mesh_ref.extract(meshlib, S.random_volume((24, 22, 20), np.uint8, 31), 128.0, S.SPACING)
        elif name == "random_u16":
            mesh = mesh_ref.extract(meshlib, S.random_volume((24, 22, 20), np.uint16, 32), 30000.0, S.SPACING)
        elif name == "ties":
            mesh = mesh_ref.extract(meshlib, S.ties_volume((24, 22, 20), 100, 33), 100.0, S.SPACING)
        elif name == "ball":
            mesh = mesh_ref.extract(meshlib, S.ball_volume(), 128.0)
        else:
            raise KeyError(name)
        for a in mesh:
            a.setflags(write=False)
        _MESHES[name] = mesh
    return _MESHES[name]


@pytest.mark.parametrize("cell", S.CELLS)
@pytest.mark.parametrize("name", ["random_u8", "random_u16", "ties", "ball"])
def test_the_restatement_is_the_numpy_statement_and_has_the_consequences(simplib, meshlib, name, cell):
    src = source_mesh(meshlib, name)
    assert src[2].shape[0] > 1000
    got, rows = simp_ref.simplify(simplib, src, cell)
    want, want_rows = S.numpy_simplify(src, cell)
    problem = M.same_bits(got, want)
    assert not problem, problem
    assert np.array_equal(rows, want_rows)
    assert S.consequences(src, got, rows, cell) == ""
    if cell == 1000.0:
        assert got[2].shape[0] == 0
    else:
        assert 0 < got[2].shape[0] <= src[2].shape[0]
    # a second simplification is the identity
    again, again_rows = simp_ref.simplify(simplib, got, cell)
    assert M.same_bits(again, got) == "" and np.array_equal(again_rows, np.arange(got[0].shape[0]))


def key_mesh(meshlib, name):
    if ("keys", name) not in _MESHES:
        make, iso, spacing = S.KEY_VOLUMES[name]
        mesh = mesh_ref.extract(meshlib, make(), float(iso), spacing)
        for a in mesh:
            a.setflags(write=False)
        _MESHES[("keys", name)] = mesh
    return _MESHES[("keys", name)]


@pytest.mark.parametrize("name,cell,bits", S.KEY_CASES, ids=S.KEY_CASE_IDS)
def test_wide_keys_and_empty_axes_are_the_numpy_statement(simplib, meshlib, name, cell, bits):
    """the cells at which an implementation that packs the three cell indices into one key needs more than 32 bits of it, all 63,
    or none for one axis.  The numpy statement's fields are 21 bits whatever the extent."""
    src = key_mesh(meshlib, name)
    if name.startswith("ties"):
        assert (src[0].shape[0], src[2].shape[0]) == (162035, 327616)
    if name == "ties":
        assert src[0].max(axis=0).tolist() == [39.0, 37.0, 35.0]
    S.assert_key_case(src[0], name, cell, bits)
    got, rows = simp_ref.simplify(simplib, src, cell)
    want, want_rows = S.numpy_simplify(src, cell)
    problem = M.same_bits(got, want)
    assert not problem, problem
    assert np.array_equal(rows, want_rows)
    assert S.consequences(src, got, rows, cell) == ""
    if name == "ties":                                      # only coincident vertices share cells this small
        assert (got[0].shape[0], got[2].shape[0]) == (99298, 220946)
    assert 0 < got[2].shape[0] < src[2].shape[0]


def test_the_ties_volume_has_coincident_vertices_that_resolve_by_index(simplib, meshlib):
    src = source_mesh(meshlib, "ties")
    pos = src[0]
    _, inverse, counts = np.unique(pos, axis=0, return_inverse=True, return_counts=True)
    assert (counts > 1).sum() > 100                           # the case exists
    got, rows = simp_ref.simplify(simplib, src, 0.3)
    # of coincident vertices only the first can be kept
    first = np.full(counts.size, pos.shape[0], dtype=np.int64)
    np.minimum.at(first, inverse.ravel(), np.arange(pos.shape[0]))
    assert np.array_equal(first[inverse.ravel()[rows]], rows)


def test_the_ball_shrinks_and_keeps_its_volume(simplib, meshlib):
    src = source_mesh(meshlib, "ball")
    assert M.closed_and_oriented(src[2]) == ""
    volume = M.signed_volume(src[0], src[2])
    assert abs(volume - 4.0 / 3.0 * np.pi * 24.0 ** 3) < 0.02 * volume
    counts = [simp_ref.simplify(simplib, src, cell)[0][2].shape[0] for cell in S.CELLS]
    assert counts[0] <= src[2].shape[0]
    assert all(a > b for a, b in zip(counts, counts[1:])), counts
    got, _ = simp_ref.simplify(simplib, src, 4.0)
    assert abs(M.signed_volume(got[0], got[2]) - volume) <= 0.02 * volume
