"""Connected components without a GPU: the C ABI's new entry points, what a host-only handle answers, known answers of the CPU
definition (tests/components_ref/components_ref.c, which tests/test_components_gpu.py holds the kernels to), that definition
against scipy.ndimage.label, and the definition's claim about the mesh: every triangle belongs to one component, so removing a
component removes rows of the mesh and changes no other byte -- which zeroing the removed voxels does not achieve."""
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


comp_ref = _load("components_ref_binding", _HERE / "components_ref" / "binding.py")
mesh_ref = _load("mesh_ref_binding", _HERE / "mesh_ref" / "binding.py")
M = _load("mesh_checks", _HERE / "mesh_checks.py")
K = _load("components_cases", _HERE / "components_cases.py")

SYMBOLS = ("vr_label_components", "vr_get_components_info", "vr_read_components", "vr_read_labels", "vr_component_at",
           "vr_select_components", "vr_select_component_list", "vr_extract_components", "vr_free_components",
           "vr_set_component_index_bits", "vr_get_components_ms")


@pytest.fixture(scope="module")
def complib(tmp_path_factory):
    return comp_ref.build(tmp_path_factory.mktemp("components_ref"))


@pytest.fixture(scope="module")
def meshlib(tmp_path_factory):
    return mesh_ref.build(tmp_path_factory.mktemp("mesh_ref_components"))


@pytest.mark.parametrize("name", SYMBOLS)
def test_library_exports_the_component_entry_points(vra, name):
    assert name in vra.symbols_declared_in_header()
    assert hasattr(C.CDLL(str(vra.LIB_PATH)), name)


def test_host_only_handle_refuses_labelling_and_has_no_components(vra):
    R = vra.renderer
    r = vra.RendererCore(-1)
    r.setup((64, 64))
    for call in (lambda: r.labelComponents(100), r.extractComponents):
        with pytest.raises(vra.VRError) as e:
            call()
        assert e.value.code == R.VR_E_NO_DEVICE
    for call in (r.componentsInfo, r.readComponents, lambda: r.componentAt(0, 0, 0), lambda: r.selectComponents(1, 0),
                 lambda: r.selectComponentList([1])):
        with pytest.raises(vra.VRError) as e:
            call()
        assert e.value.code == R.VR_E_INVALID
    for bits in (0, 32, 64):
        r.setComponentIndexBits(bits)
    with pytest.raises(vra.VRError) as e:
        r.setComponentIndexBits(16)
    assert e.value.code == R.VR_E_INVALID
    r.setComponentIndexBits(0)
    r.freeComponents()                                    # nothing to free is not an error
    assert r.componentsMs() == 0.0
    r.close()


# ---------------------------------------------------------------- known answers of the restatement
def test_nothing_inside_and_everything_inside(complib):
    vol = np.full((6, 11, 13), 7, dtype=np.uint8)
    labels, rec = comp_ref.label(complib, vol, 8.0)
    assert rec["voxels"].size == 0 and not labels.any()
    labels, rec = comp_ref.label(complib, vol, 7.0)
    assert np.all(labels == 1)
    assert rec["voxels"].tolist() == [13 * 11 * 6] and rec["first_voxel"].tolist() == [0]
    assert rec["bbox"].tolist() == [[0, 0, 0, 12, 10, 5]]


@pytest.mark.parametrize("e", K.DIRS, ids=str)
def test_a_pair_along_one_of_the_seven_directions_is_one_component(complib, e):
    labels, rec = comp_ref.label(complib, K.pair_volume(e), K.ISO)
    assert rec["voxels"].tolist() == [2]
    assert rec["bbox"].tolist() == [[2, 2, 2, 2 + e[0], 2 + e[1], 2 + e[2]]]
    assert rec["first_voxel"].tolist() == [2 + 5 * (2 + 5 * 2)]


@pytest.mark.parametrize("e", K.NON_ADJACENT, ids=str)
def test_a_pair_along_another_diagonal_is_two_components(complib, e):
    vol = K.pair_volume(e)
    labels, rec = comp_ref.label(complib, vol, K.ISO)
    assert rec["voxels"].tolist() == [1, 1]
    first = sorted([2 + 5 * (2 + 5 * 2), (2 + e[0]) + 5 * ((2 + e[1]) + 5 * (2 + e[2]))])
    assert rec["first_voxel"].tolist() == first           # numbered by first voxel
    assert labels.reshape(-1)[first[0]] == 1 and labels.reshape(-1)[first[1]] == 2


def test_a_ball_inside_a_hollow_sphere(complib):
    vol = K.nested_shells()
    labels, rec = comp_ref.label(complib, vol, K.ISO)
    assert rec["voxels"].size == 2
    c = vol.shape[0] // 2
    assert labels[c, c, c] == 2 and labels[c, c, c + 11] == 1 and labels[c, c, c + 7] == 0
    assert rec["first_voxel"][0] < rec["first_voxel"][1]
    assert rec["bbox"].tolist() == [[c - 12, c - 12, c - 12, c + 12, c + 12, c + 12], [c - 5, c - 5, c - 5, c + 5, c + 5, c + 5]]
    assert int(rec["voxels"].sum()) == int((vol == K.ON).sum())


def test_a_serpentine_is_one_component_of_the_known_length(complib):
    vol, length = K.serpentine(40)
    labels, rec = comp_ref.label(complib, vol, K.ISO)
    assert rec["voxels"].tolist() == [length] and rec["first_voxel"].tolist() == [0]
    assert rec["bbox"].tolist() == [[0, 0, 0, 39, 38, 38]]


def test_the_selection_rule(complib):
    voxels = np.array([5, 9, 1, 9, 3, 5], dtype=np.uint64)
    assert comp_ref.select(complib, voxels, 0, 0).all()
    assert comp_ref.select(complib, voxels, 4, 0).tolist() == [True, True, False, True, False, True]
    assert comp_ref.select(complib, voxels, 0, 1).tolist() == [False, True, False, False, False, False]     # ties: the lower label
    assert comp_ref.select(complib, voxels, 0, 3).tolist() == [True, True, False, True, False, False]
    assert comp_ref.select(complib, voxels, 6, 3).tolist() == [False, True, False, True, False, False]
    assert comp_ref.select(complib, voxels, 0, 99).all()


RANDOM_SHAPES = [(13, 11, 6), (33, 17, 9), (70, 66, 68)]
RANDOM_CASES = [(s, d, iso) for s in RANDOM_SHAPES for d, isos in ((np.uint8, (128, 200, 220)), (np.uint16, (8000, 60000))) for iso in isos]


def random_volume(shape_xyz, dtype, seed):
    nx, ny, nz = shape_xyz
    hi = 256 if dtype == np.uint8 else 65536
    return np.random.default_rng(seed).integers(0, hi, size=(nz, ny, nx)).astype(dtype)


def test_the_restatement_against_scipy(complib):
    ndimage = pytest.importorskip("scipy.ndimage")
    structure = np.zeros((3, 3, 3), dtype=bool)
    structure[1, 1, 1] = True
    for dx, dy, dz in K.DIRS:
        structure[1 + dz, 1 + dy, 1 + dx] = structure[1 - dz, 1 - dy, 1 - dx] = True
    assert structure.sum() == 15                          # the voxel and its 14 neighbours
    vols = [(random_volume(s, d, sum(s)), float(iso)) for s, d, iso in RANDOM_CASES]
    vols += [(K.nested_shells(), K.ISO), (K.serpentine(40)[0], K.ISO), (K.checkerboard(), K.ISO), (K.seam_pairs()[0], K.ISO)]
    for vol, iso_s in vols:
        labels, rec = comp_ref.label(complib, vol, iso_s)
        lab, n = ndimage.label(vol.astype(np.float32) >= np.float32(iso_s), structure=structure)
        assert n == rec["voxels"].size
        assert np.array_equal(K.renumber_by_first_voxel(lab), labels)
        assert np.array_equal(np.bincount(labels.reshape(-1), minlength=n + 1)[1:], rec["voxels"].astype(np.int64))


def test_the_seam_volume_has_its_closed_form_count(complib):
    vol, components = K.seam_pairs()
    assert components == 5 * (4 * 3 + 2 * (2 + 2 + 2 + 3 + 3 + 3))
    labels, rec = comp_ref.label(complib, vol, K.ISO)
    assert rec["voxels"].size == components and int(rec["voxels"].sum()) == int((vol == K.ON).sum())


# ---------------------------------------------------------------- the definition's claim about the mesh
@pytest.mark.parametrize("shape,dtype,iso", RANDOM_CASES, ids=lambda v: getattr(v, "__name__", str(v)))
def test_every_triangle_belongs_to_one_component_and_removal_removes_rows(complib, meshlib, shape, dtype, iso):
    vol = random_volume(shape, dtype, sum(shape))
    iso_s = float(iso)
    spacing = (0.5, 1.0, 2.0)
    labels, rec = comp_ref.label(complib, vol, iso_s)
    n = rec["voxels"].size
    assert n >= 1
    full = mesh_ref.extract(meshlib, vol, iso_s, spacing)
    vlabel = K.vertex_labels(vol.astype(np.float32) >= np.float32(iso_s), labels)
    assert vlabel.shape[0] == full[0].shape[0]
    tl = vlabel[full[2].astype(np.int64)]
    assert np.all(tl[:, 0] == tl[:, 1]) and np.all(tl[:, 0] == tl[:, 2])
    # every component selected: the filtered extraction is the extraction
    assert M.same_bits(comp_ref.extract(complib, vol, iso_s, labels, rec["selected"], spacing), full) == ""
    # "at least 3 voxels": the kept rows of the full mesh, bit for bit
    sel = comp_ref.select(complib, rec["voxels"], 3, 0)
    assert np.array_equal(sel, rec["voxels"] >= 3)
    got = comp_ref.extract(complib, vol, iso_s, labels, sel, spacing)
    want = K.sub_mesh(full, vlabel, sel)
    assert M.same_bits(got, want) == ""
    if sel.all() or not sel.any():
        return
    # zeroing the removed voxels and extracting again: the same positions and triangles, but not the same normals
    zeroed = np.where((labels != 0) & ~np.concatenate([[False], sel])[labels], 0, vol).astype(dtype)
    again = mesh_ref.extract(meshlib, zeroed, iso_s, spacing)
    assert M.same_bits((again[0], again[0], again[2]), (want[0], want[0], want[2])) == ""
    assert again[1].shape == want[1].shape and not np.array_equal(again[1].view(np.uint32), want[1].view(np.uint32))
