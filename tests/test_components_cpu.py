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


# ---------------------------------------------------------------- volumes for the branches no random volume reaches
# (tests/test_components_gpu.py runs the kernels on them; here the restatement has its known answers and the cases exist)
def linear_of(vol):
    return np.flatnonzero(vol.reshape(-1))


def xyz_of(lin, vol):
    nz, ny, nx = vol.shape
    return np.stack([lin % nx, lin // nx % ny, lin // (nx * ny)], axis=1)


def test_the_lattice_is_one_component_per_voxel(complib):
    vol = K.lattice((64, 16, 16))
    labels, rec = comp_ref.label(complib, vol, K.ISO)
    lin = linear_of(vol)
    assert lin.size == 4096 == rec["voxels"].size and np.all(rec["voxels"] == 1)
    assert np.array_equal(rec["first_voxel"], lin.astype(np.uint64))           # ascending linear order
    at = xyz_of(lin, vol)
    assert np.array_equal(rec["bbox"][:, :3], at) and np.array_equal(rec["bbox"][:, 3:], at)
    assert np.array_equal(labels.reshape(-1)[lin], np.arange(1, 4097))
    assert K.labels_per_chunk(labels).tolist() == [2048, 2048]


@pytest.mark.parametrize("n", [1023, 1024, 1025, 2048])
def test_the_first_n_lattice_voxels_of_every_chunk(complib, n):
    full = K.lattice((64, 16, 16))
    vol = K.first_n_per_chunk(full, n)
    assert np.all((vol == 0) | (vol == full)) and (n < 2048 or np.array_equal(vol, full))
    flat = vol.reshape(-1)
    for at in (0, K.CHUNK):                                 # the first n of each chunk, not any n
        assert np.array_equal(np.flatnonzero(flat[at:at + K.CHUNK]), np.flatnonzero(full.reshape(-1)[at:at + K.CHUNK])[:n])
    labels, rec = comp_ref.label(complib, vol, K.ISO)
    assert rec["voxels"].size == 2 * n and np.all(rec["voxels"] == 1)
    assert K.labels_per_chunk(labels).tolist() == [n, n]


def test_y_lines_are_two_runs_of_one_component_in_one_chunk(complib):
    vol = K.y_lines()
    nz, ny, nx = vol.shape
    assert nx * ny == K.CHUNK
    labels, rec = comp_ref.label(complib, vol, K.ISO)
    assert rec["voxels"].size == 4096 and np.all(rec["voxels"] == 2)
    bb = rec["bbox"]
    assert np.all(bb[:, 1] == 0) and np.all(bb[:, 4] == 1) and np.array_equal(bb[:, 0], bb[:, 3]) and np.array_equal(bb[:, 2], bb[:, 5])
    assert np.all(bb[:, 0] % 2 == 0) and np.all(bb[:, 2] % 2 == 0)
    assert np.array_equal(labels[:, 0, :], labels[:, 1, :])                   # the two voxels of a column, nx apart
    per = K.labels_per_chunk(labels)
    assert per.tolist() == [2048, 0, 2048, 0] and per.max() > K.REC_SLOTS


def test_the_odd_lattice_has_chunks_that_cut_rows(complib):
    vol = K.lattice((13, 11, 120))
    assert K.CHUNK % 13 != 0
    labels, rec = comp_ref.label(complib, vol, K.ISO)
    assert rec["voxels"].size == int((vol == K.ON).sum()) and np.all(rec["voxels"] == 1)
    assert K.labels_per_chunk(labels).max() > K.REC_SLOTS


@pytest.mark.parametrize("stem_from", [0, 6])
def test_the_lattice_under_a_slab_shares_a_chunk_with_it(complib, stem_from):
    vol = K.lattice_under_a_slab(stem_from)
    labels, rec = comp_ref.label(complib, vol, K.ISO)
    assert rec["voxels"].size == 1536 + 1
    slab = int(labels[-1, -1, -1])
    assert rec["voxels"][slab - 1] == 64 * 16 * 14 + 64 * 3 * (10 - stem_from) and np.all(np.delete(rec["voxels"], slab - 1) == 1)
    assert rec["bbox"][slab - 1].tolist() == [0, 0, stem_from, 63, 15, 23]
    first = labels.reshape(-1)[:K.CHUNK]
    assert K.labels_per_chunk(labels)[0] == 1537 and slab in first              # more than a table of them, the slab's among them
    # labels number the components by first voxel: how many the first chunk holds before the slab's first run
    assert slab - 1 == 192 * (stem_from + 1)
    assert (slab - 1 < K.REC_SLOTS) == (stem_from == 0)
    assert np.unique(labels.reshape(-1)[K.CHUNK:]).tolist() == [0, slab]        # ... and it goes on alone through the next chunks


@pytest.mark.parametrize("second_block", [False, True], ids=["one block", "two blocks"])
def test_a_solid_with_a_hole_has_whole_tiles(complib, second_block):
    vol = K.solid_with_hole(second_block=second_block)
    inside = vol == K.ON
    labels, rec = comp_ref.label(complib, vol, K.ISO)
    assert rec["voxels"].size == 1 + second_block
    assert rec["voxels"].tolist() == [int((inside & (labels == c)).sum()) for c in range(1, 2 + second_block)]
    assert int(rec["voxels"].sum()) == int(inside.sum())
    assert rec["first_voxel"][0] == 0 and rec["bbox"][0].tolist() == [0, 0, 0, 69, 65, 67]
    if second_block:
        assert rec["voxels"][1] == 60 * 52 * 20 and rec["bbox"][1].tolist() == [5, 7, 42, 64, 58, 61]
        assert K.full_tiles(labels == 1) > 0 and K.full_tiles(labels == 2) == 1 * 6 * 4
    else:
        assert rec["voxels"].tolist() == [70 * 66 * 68 - 50 * 20 * 4] == [310160]
        assert K.full_tiles(inside) == 260


def test_full_tiles_counts_aligned_tiles_inside_the_volume():
    assert K.full_tiles(np.ones((4, 8, 32), dtype=bool)) == 1
    assert K.full_tiles(np.ones((7, 15, 63), dtype=bool)) == 1 and K.full_tiles(np.ones((3, 8, 32), dtype=bool)) == 0
    inside = np.ones((8, 16, 64), dtype=bool)
    assert K.full_tiles(inside) == 8
    inside[5, 9, 40] = False
    assert K.full_tiles(inside) == 7
    shifted = np.zeros((8, 16, 64), dtype=bool)
    shifted[1:5, 1:9, 1:33] = True                          # a tile's worth, not on the tiles' grid
    assert K.full_tiles(shifted) == 0


def test_no_other_gpu_volume_overfills_a_table_or_fills_a_tile(complib):
    """What the new volumes are for: of the volumes tests/test_components_gpu.py had before them, none puts more than 1024
    labels into an 8192-voxel chunk and none holds a whole tile of inside voxels."""
    vols = []
    for dtype, isos in ((np.uint8, (40, 128, 220)), (np.uint16, (8000, 30000, 60000))):
        vol = random_volume((70, 66, 68), dtype, 70 + 66 + 68 + np.dtype(dtype).itemsize)
        vols += [(vol, comp_ref.iso_stored(iso, dtype, True)) for iso in isos]
    vols += [(K.nested_shells(), K.ISO), (K.comb()[0], K.ISO)]
    for vol, iso_s in vols:
        labels, rec = comp_ref.label(complib, vol, iso_s)
        assert K.labels_per_chunk(labels).max() <= K.REC_SLOTS
        assert K.full_tiles(vol.astype(np.float32) >= np.float32(iso_s)) == 0


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
