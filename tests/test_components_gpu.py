"""vr_label_components, the selection and vr_extract_components on the device against their CPU definition
(tests/components_ref/components_ref.c), bit for bit as arrays: both voxel types, both layouts, shapes that are no multiple of a
tile or hold a single voxel; pairs across every kind of tile boundary; a serpentine, a comb, a checkerboard and nested shells;
the 64-bit parents; the filtered extraction as the restatement's and as the numpy sub-mesh of the device's own full mesh, in one
piece and in z slabs; what the labelling does to the handle's state; chunks with more labels than the records pass's table holds;
and solid regions, whose whole tiles skip the tile pass's unions."""
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


comp_ref = _load("components_ref_binding", _HERE / "components_ref" / "binding.py")
M = _load("mesh_checks", _HERE / "mesh_checks.py")
K = _load("components_cases", _HERE / "components_cases.py")

SHAPES = [(13, 11, 6), (70, 66, 68), (130, 9, 5), (5, 3, 2), (64, 2, 2), (5, 3, 1), (1, 1, 1)]          # (nx, ny, nz)
ISOS = {np.uint8: (40, 128, 220), np.uint16: (8000, 30000, 60000)}
SPACING = (0.5, 1.0, 2.0)
LAYOUTS = pytest.mark.parametrize("layout", [0, 1], ids=["linear", "bricked"])
DTYPES = pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])


@pytest.fixture(scope="module")
def complib(tmp_path_factory):
    return comp_ref.build(tmp_path_factory.mktemp("components_ref_gpu"))


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


def reference(complib, key, vol, iso_s):
    """the CPU definition's labels and records, computed once per (volume key, iso_s) and shared"""
    k = (key, float(iso_s))
    if k not in _REF:
        labels, rec = comp_ref.label(complib, vol, iso_s)
        labels.setflags(write=False)
        for a in rec.values():
            a.setflags(write=False)
        _REF[k] = (labels, rec)
    return _REF[k]


def assert_same_labelling(r, want, what, selected=None):
    labels, rec = want
    n = rec["voxels"].size
    info = r.componentsInfo()
    sel = rec["selected"] if selected is None else selected
    assert (info["components"], info["inside"], info["selected"]) == (n, int(rec["voxels"].sum()), int(sel.sum())), what
    got = r.readComponents()
    for name in ("voxels", "first_voxel", "bbox"):
        assert got[name].dtype == rec[name].dtype and np.array_equal(got[name], rec[name]), f"{what}: {name}"
    assert np.array_equal(got["selected"], sel), f"{what}: selected"
    assert np.array_equal(r.readLabels(), labels), f"{what}: labels"


def assert_same_mesh(got, want, what):
    problem = M.same_bits(got, want)
    assert not problem, f"{what}: {problem}"


# ---------------------------------------------------------------- 1. labels, records, n_inside
@DTYPES
@LAYOUTS
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_labels_and_records_match_the_reference(vra, complib, handle, shape, layout, dtype):
    R = vra.renderer
    r = handle
    seed = sum(shape) + np.dtype(dtype).itemsize
    vol = random_volume(shape, dtype, seed)
    r.setComponentIndexBits(0)
    r.setLayout(layout)
    r.setQuirks(R.QUIRK_DEFAULT)
    r.setVolume(vol, SPACING)
    for iso in ISOS[dtype]:
        n = r.labelComponents(iso)
        want = reference(complib, (shape, seed), vol, comp_ref.iso_stored(iso, dtype, True))
        assert n == want[1]["voxels"].size and r.componentsInfo()["iso"] == iso
        assert_same_labelling(r, want, f"iso {iso}")
    if dtype == np.uint16:                                  # without the quirk the same number means other voxels
        r.setQuirks(0)
        iso = ISOS[dtype][1]
        r.labelComponents(iso)
        assert_same_labelling(r, reference(complib, (shape, seed), vol, float(iso)), "quirk off")
        r.setQuirks(R.QUIRK_DEFAULT)


# ---------------------------------------------------------------- 2. seams
@pytest.fixture(scope="module")
def seams():
    vol, components = K.seam_pairs()
    vol.setflags(write=False)
    return vol, components


@LAYOUTS
def test_pairs_across_every_kind_of_tile_boundary(vra, complib, handle, seams, layout):
    r = handle
    vol, components = seams
    r.setComponentIndexBits(0)
    r.setLayout(layout)
    r.setVolume(vol)
    assert r.labelComponents(K.ISO) == components == 210
    assert_same_labelling(r, reference(complib, "seams", vol, K.ISO), "seam pairs")


# ---------------------------------------------------------------- 3. structures
STRUCTURES = {
    "serpentine": lambda: K.serpentine(40)[0],
    "comb": lambda: K.comb()[0],
    "checkerboard": K.checkerboard,
    "shells": K.nested_shells,
}


@LAYOUTS
@pytest.mark.parametrize("name", sorted(STRUCTURES))
def test_structures(vra, complib, handle, name, layout):
    r = handle
    vol = STRUCTURES[name]()
    r.setComponentIndexBits(0)
    r.setLayout(layout)
    r.setVolume(vol)
    n = r.labelComponents(K.ISO)
    want = reference(complib, name, vol, K.ISO)
    assert n == want[1]["voxels"].size
    if name in ("serpentine", "comb"):
        assert n == 1 and r.readComponents()["voxels"].tolist() == [int((vol == K.ON).sum())]
    if name == "shells":
        assert n == 2
    assert_same_labelling(r, want, name)


def test_a_volume_whose_grids_have_a_second_row(vra, complib, handle):
    """336 x 320 x 320 voxels, more than 2^25: the launches of every kernel -- per voxel, per tile and the records' 8192-voxel
    pieces -- are two-dimensional grids with more than one row.  Noise in the first and the last eight planes, zeros between."""
    r = handle
    nx, ny, nz = 336, 320, 320
    assert nx * ny * nz > 2 ** 25
    vol = np.zeros((nz, ny, nx), dtype=np.uint8)
    rng = np.random.default_rng(21)
    vol[:8] = rng.integers(0, 256, size=(8, ny, nx))
    vol[-8:] = rng.integers(0, 256, size=(8, ny, nx))
    want = comp_ref.label(complib, vol, 215.0)
    assert want[1]["voxels"].size > 1000 and want[1]["first_voxel"][-1] > 2 ** 25
    r.setLayout(vra.renderer.LAYOUT_BRICKED)
    r.setVolume(vol)
    try:
        for bits in (0, 64):
            r.setComponentIndexBits(bits)
            assert r.labelComponents(215) == want[1]["voxels"].size
            assert_same_labelling(r, want, f"{bits}-bit parents")
        r.selectComponents(0, 1)
        nv, nt = r.extractComponents()                      # the selection plane's kernel
        assert nt > 0
    finally:
        r.setComponentIndexBits(0)
        r.freeMesh()
        r.freeComponents()


# ---------------------------------------------------------------- 4. the wide instance
@LAYOUTS
def test_64_bit_parents_give_the_same_bytes(vra, complib, handle, seams, layout):
    r = handle
    r.setLayout(layout)
    try:
        r.setComponentIndexBits(64)
        shape, dtype = (70, 66, 68), np.uint16
        seed = sum(shape) + 2
        vol = random_volume(shape, dtype, seed)
        r.setVolume(vol, SPACING)
        for iso in ISOS[dtype]:
            r.labelComponents(iso)
            assert_same_labelling(r, reference(complib, (shape, seed), vol, comp_ref.iso_stored(iso, dtype, True)), f"wide, iso {iso}")
        r.setVolume(seams[0])
        assert r.labelComponents(K.ISO) == seams[1]
        assert_same_labelling(r, reference(complib, "seams", seams[0], K.ISO), "wide, seam pairs")
        vol = K.serpentine(40)[0]
        r.setVolume(vol)
        assert r.labelComponents(K.ISO) == 1
        assert_same_labelling(r, reference(complib, "serpentine", vol, K.ISO), "wide, serpentine")
    finally:
        r.setComponentIndexBits(0)


# ---------------------------------------------------------------- 5. filtered extraction
@DTYPES
@LAYOUTS
def test_filtered_extraction(vra, complib, handle, layout, dtype, tmp_path):
    r = handle
    shape = (70, 66, 68)
    seed = sum(shape) + np.dtype(dtype).itemsize
    vol = random_volume(shape, dtype, seed)
    iso = ISOS[dtype][2]                                    # sparse: thousands of components, many of one or two voxels
    iso_s = comp_ref.iso_stored(iso, dtype, True)
    r.setComponentIndexBits(0)
    r.setLayout(layout)
    r.setQuirks(vra.renderer.QUIRK_DEFAULT)
    r.setVolume(vol, SPACING)
    r.setMeshWorkspace(0)
    r.extractIsosurface(iso)
    full = r.readMesh()
    n = r.labelComponents(iso)
    labels, rec = reference(complib, (shape, seed), vol, iso_s)
    assert n == rec["voxels"].size > 100
    # every component selected: extractIsosurface's mesh byte for byte
    assert r.extractComponents() == (full[0].shape[0], full[2].shape[0])
    assert r.meshInfo() == dict(iso=iso, vertices=full[0].shape[0], triangles=full[2].shape[0])
    assert_same_mesh(r.readMesh(), full, "everything selected")
    vlabel = K.vertex_labels(vol.astype(np.float32) >= np.float32(iso_s), r.readLabels())
    assert vlabel.shape[0] == full[0].shape[0]
    plane = 9 * shape[0] * shape[1]
    for min_voxels, keep in ((3, 0), (0, 1), (0, 2), (3, 2)):
        sel = comp_ref.select(complib, rec["voxels"], min_voxels, keep)
        assert r.selectComponents(min_voxels, keep) == int(sel.sum())
        assert np.array_equal(r.readComponents()["selected"], sel)
        if keep:                                            # ties go to the lower label
            order = sorted(range(n), key=lambda c: (-int(rec["voxels"][c]), c))
            assert set(np.flatnonzero(sel).tolist()) <= set(order[:keep])
        nv, nt = r.extractComponents()
        got = r.readMesh()
        assert (nv, nt) == (got[0].shape[0], got[2].shape[0]) and 0 < nt < full[2].shape[0]
        assert_same_mesh(got, comp_ref.extract(complib, vol, iso_s, labels, sel, SPACING), f"restatement, {min_voxels}/{keep}")
        assert_same_mesh(got, K.sub_mesh(full, vlabel, sel), f"sub-mesh of the full mesh, {min_voxels}/{keep}")
        if (min_voxels, keep) == (3, 0):
            try:
                for planes in (2, 8):                       # z slabs of 1 and 7 planes
                    r.setMeshWorkspace(planes * plane + plane // 2)
                    assert r.extractComponents() == (nv, nt)
                    assert_same_mesh(r.readMesh(), got, f"{planes} planes of work arrays")
            finally:
                r.setMeshWorkspace(0)
            r.saveMesh(tmp_path / "kept.ply", "ply")
            raw = (tmp_path / "kept.ply").read_bytes()
            assert f"element vertex {nv}\n".encode() in raw and f"element face {nt}\n".encode() in raw
            end = raw.index(b"end_header\n") + len(b"end_header\n")
            verts = np.frombuffer(raw, dtype="<f4", count=6 * nv, offset=end).reshape(nv, 6)
            assert np.array_equal(verts[:, :3].view(np.uint32), got[0].view(np.uint32))
    # nothing selected: the empty mesh, and the call succeeds
    assert r.selectComponentList([]) == 0
    assert r.extractComponents() == (0, 0) and r.meshInfo() == dict(iso=iso, vertices=0, triangles=0)
    # a list
    some = [1, n, n // 2]
    assert r.selectComponentList(some) == 3
    sel = np.zeros(n, dtype=bool)
    sel[np.array(some) - 1] = True
    r.extractComponents()
    assert_same_mesh(r.readMesh(), K.sub_mesh(full, vlabel, sel), "a list of labels")


@LAYOUTS
def test_the_inner_ball_alone_is_a_closed_sphere(vra, handle, layout):
    r = handle
    r.setComponentIndexBits(0)
    r.setLayout(layout)
    r.setVolume(K.nested_shells())
    assert r.labelComponents(K.ISO) == 2
    c = 33 // 2
    assert r.componentAt(c, c, c) == 2 and r.componentAt(c + 11, c, c) == 1 and r.componentAt(c + 7, c, c) == 0
    assert r.selectComponentList([2]) == 1
    nv, nt = r.extractComponents()
    pos, nrm, tri = r.readMesh()
    assert nt > 0 and M.closed_and_oriented(tri) == "" and M.every_vertex_referenced(nv, tri)
    assert M.euler_characteristic(nv, tri) == 2 and M.signed_volume(pos, tri) > 0
    assert np.all(np.abs(pos - c).max(axis=1) <= 5.5)
    r.selectComponents(0, 0)
    nv, nt = r.extractComponents()
    assert M.euler_characteristic(nv, r.readMesh()[2]) == 6          # the ball and the shell's two spheres


# ---------------------------------------------------------------- 6. state
def frame(r):
    r.render()
    rgba = r.readPixels().copy()
    total, spp = r.countSamples(per_pixel=True)
    return rgba, spp.copy(), total


def test_labelling_leaves_the_renderer_alone_and_belongs_to_the_voxels(vra, oracle, complib, handle):
    r = handle
    R = vra.renderer
    dims = (41, 39, 40)
    vol = oracle.gen_noise_ball(dims, 2, 77)
    iso = (int(vol.min()) + int(vol.max())) // 2 - 1000
    r.setComponentIndexBits(0)
    r.setLayout(R.LAYOUT_BRICKED)
    r.setQuirks(R.QUIRK_DEFAULT)
    r.setVolume(vol)
    r.freeMesh()
    r.freeComponents()
    for call in (r.componentsInfo, r.readLabels, r.extractComponents, lambda: r.selectComponents(1, 0), lambda: r.componentAt(0, 0, 0)):
        with pytest.raises(vra.VRError) as e:
            call()
        assert e.value.code == R.VR_E_INVALID
    before = frame(r)
    r.takeMessage()
    state = (r.window, r.residentBytes()[:2], bits(r.getCameraBlock()).tolist(), r.smoothing)
    other, choice, kernel = r.residentBytes()[2], r.last_launch_choice, r.last_kernel_name
    n = r.labelComponents(iso)
    assert n >= 1 and r.takeMessage() is None and r.componentsMs() > 0.0
    assert r.residentBytes()[2] == other + 4 * vol.size             # the labels count under `other`
    want = reference(complib, "ball16", vol, float(iso + 1000))
    assert_same_labelling(r, want, "noise ball")
    r.selectComponents(0, 1)
    nv, nt = r.extractComponents()
    assert nt > 0
    assert (r.last_launch_choice, r.last_kernel_name) == (choice, kernel)
    assert (r.window, r.residentBytes()[:2], bits(r.getCameraBlock()).tolist(), r.smoothing) == state
    assert r.residentBytes()[2] == other + 4 * vol.size + 24 * nv + 12 * nt
    got = frame(r)
    assert np.array_equal(bits(got[0]), bits(before[0])) and np.array_equal(got[1], before[1]) and got[2] == before[2]
    # componentAt agrees with readLabels
    labels = r.readLabels()
    rng = np.random.default_rng(3)
    for i, j, k in zip(rng.integers(0, dims[0], 12), rng.integers(0, dims[1], 12), rng.integers(0, dims[2], 12)):
        assert r.componentAt(i, j, k) == labels[k, j, i]
    # bad arguments change nothing
    lib = vra.load_library()
    sel = r.readComponents()["selected"].copy()
    for bad in ([0], [n + 1], [1, n + 7]):
        with pytest.raises(vra.VRError) as e:
            r.selectComponentList(bad)
        assert e.value.code == R.VR_E_INVALID
    for bad in ((-1, 0, 0), (dims[0], 0, 0), (0, dims[1], 0), (0, 0, dims[2])):
        with pytest.raises(vra.VRError) as e:
            r.componentAt(*bad)
        assert e.value.code == R.VR_E_INVALID
    small = np.zeros(vol.size - 1, dtype=np.uint32)
    assert lib.vr_read_labels(r._h, small.ctypes.data_as(C.POINTER(C.c_uint32)), small.size) == R.VR_E_INVALID
    if n > 1:
        few = np.zeros(n - 1, dtype=np.uint64)
        assert lib.vr_read_components(r._h, few.ctypes.data_as(C.POINTER(C.c_uint64)), None, None, None, n - 1) == R.VR_E_INVALID
    assert lib.vr_read_components(r._h, None, None, None, None, 0) == R.VR_OK
    assert np.array_equal(r.readComponents()["selected"], sel)
    assert_same_labelling(r, want, "after refused calls", selected=sel)
    # kept across the layout and the quirks (it stores its iso_s); the extraction after them is the same bytes
    mesh = r.readMesh()
    r.setLayout(R.LAYOUT_LINEAR)
    r.setQuirks(0)
    assert_same_labelling(r, want, "after setLayout and setQuirks", selected=sel)
    assert r.extractComponents() == (nv, nt) and r.meshInfo()["iso"] == iso
    assert_same_mesh(r.readMesh(), mesh, "after setLayout and setQuirks")
    r.setQuirks(R.QUIRK_DEFAULT)
    r.setLayout(R.LAYOUT_BRICKED)
    # smoothing drops it; the new labelling is the smoothed volume's
    r.smoothVolume(sigma_voxels=(1.0, 1.0, 1.0))
    with pytest.raises(vra.VRError) as e:
        r.extractComponents()
    assert e.value.code == R.VR_E_INVALID
    assert_same_mesh(r.readMesh(), mesh, "the mesh stays")
    smoothed = r.readVolume()
    r.labelComponents(iso)
    assert_same_labelling(r, comp_ref.label(complib, smoothed, float(iso + 1000)), "smoothed")
    r.smoothVolume(sigma_voxels=0.0)
    with pytest.raises(vra.VRError):
        r.componentsInfo()
    # ... and so do setVolume and generateSynthetic
    r.labelComponents(iso)
    r.setVolume(random_volume((9, 8, 7), np.uint16, 1))
    with pytest.raises(vra.VRError) as e:
        r.extractComponents()
    assert e.value.code == R.VR_E_INVALID
    r.labelComponents(30000)
    r.generateSynthetic(0, (16, 16, 16), 1, 6)
    with pytest.raises(vra.VRError) as e:
        r.extractComponents()
    assert e.value.code == R.VR_E_INVALID
    # freeComponents gives the bytes back
    r.freeMesh()
    base = r.residentBytes()[2]
    r.labelComponents(100)
    assert r.residentBytes()[2] == base + 4 * 16 ** 3
    r.freeComponents()
    assert r.residentBytes()[2] == base
    fresh = vra.RendererCore(0)
    try:
        fresh.setup((64, 48))
        with pytest.raises(vra.VRError) as e:
            fresh.labelComponents(100)                      # before any volume: what vr_read_volume gives
        assert e.value.code == R.VR_E_INVALID
    finally:
        fresh.close()


# ---------------------------------------------------------------- 7. more labels in a chunk than the records' table holds
WIDTHS = pytest.mark.parametrize("index_bits", [0, 64], ids=["auto", "wide"])
# name -> (volume, the most labels one 8192-voxel chunk holds; None: more than the table's 1024, however many)
CROWDED = {
    "lattice": (lambda: K.lattice((64, 16, 16)), 2048),
    "first 1023": (lambda: K.first_n_per_chunk(K.lattice((64, 16, 16)), 1023), 1023),       # the table's last slot stays free
    "first 1024": (lambda: K.first_n_per_chunk(K.lattice((64, 16, 16)), 1024), 1024),       # exactly full, nothing goes direct
    "first 1025": (lambda: K.first_n_per_chunk(K.lattice((64, 16, 16)), 1025), 1025),       # one label a chunk goes direct
    "first 2048": (lambda: K.first_n_per_chunk(K.lattice((64, 16, 16)), 2048), 2048),
    "y lines": (K.y_lines, 2048),                           # two runs a label, the table full between them or before both
    "odd lattice": (lambda: K.lattice((13, 11, 120)), None),        # chunks cut rows; nx odd: scalar parent stores
    "slab early": (lambda: K.lattice_under_a_slab(0), 1537),        # a large component in the table, one-voxel ones direct
    "slab late": (lambda: K.lattice_under_a_slab(6), 1537),         # ... and the large one's runs meeting a full table
}


def label_and_compare(r, complib, key, vol, layout, index_bits, iso=K.ISO, iso_s=K.ISO, most=None, check=None):
    """the labelling of `vol` on the device against the restatement's; `most`: what the restatement says of the chunks, asserted
    before the device is asked; `check(labels, rec)`: further conditions on the input"""
    want = reference(complib, key, vol, iso_s)
    per = K.labels_per_chunk(want[0])
    assert per.max() > K.REC_SLOTS if most is None else per.max() == most, per.tolist()
    if check is not None:
        check(*want)
    try:
        r.setComponentIndexBits(index_bits)
        r.setLayout(layout)
        r.setVolume(vol)
        assert r.labelComponents(iso) == want[1]["voxels"].size
        assert_same_labelling(r, want, f"{key}, {index_bits}-bit parents")
    finally:
        r.setComponentIndexBits(0)
    return want


@WIDTHS
@LAYOUTS
@pytest.mark.parametrize("name", sorted(CROWDED))
def test_chunks_with_more_labels_than_the_table_holds(vra, complib, handle, name, layout, index_bits):
    make, most = CROWDED[name]
    vol = make()

    def check(labels, rec):
        if name.startswith("slab"):                         # the large component shares the crowded chunk
            slab = int(labels[-1, -1, -1])
            assert rec["voxels"][slab - 1] > 10000 and slab in labels.reshape(-1)[:K.CHUNK]
            assert K.labels_per_chunk(labels)[0] > K.REC_SLOTS
            assert (slab - 1 < K.REC_SLOTS) == (name == "slab early")
        if name == "y lines":
            assert np.all(rec["voxels"] == 2) and np.array_equal(labels[:, 0, :], labels[:, 1, :])

    label_and_compare(handle, complib, name, vol, layout, index_bits, most=most, check=check)


@LAYOUTS
def test_a_16_bit_lattice_through_the_offset(vra, complib, handle, layout):
    r = handle
    vol = np.where(K.lattice((64, 16, 16)) != 0, 40000, 0).astype(np.uint16)
    r.setQuirks(vra.renderer.QUIRK_DEFAULT)
    iso_s = comp_ref.iso_stored(20000, np.uint16, True)
    assert iso_s == 21000.0
    label_and_compare(r, complib, "lattice16", vol, layout, 0, iso=20000, iso_s=iso_s, most=2048)


# ---------------------------------------------------------------- 8. whole tiles of inside voxels
def on_off(vol, dtype):
    """a volume of 0 / K.ON as `dtype`, the iso to label it at and that iso in stored units (16-bit: 0 / 40000 at 20000, which
    the offset moves to 21000)"""
    if dtype == np.uint8:
        return vol.astype(np.uint8), K.ISO, float(K.ISO)
    return np.where(vol != 0, 40000, 0).astype(np.uint16), 20000, comp_ref.iso_stored(20000, np.uint16, True)


@DTYPES
@WIDTHS
@LAYOUTS
@pytest.mark.parametrize("second_block", [False, True], ids=["one block", "two blocks"])
def test_a_solid_with_a_hole(vra, complib, handle, second_block, layout, index_bits, dtype):
    r = handle
    vol, iso, iso_s = on_off(K.solid_with_hole(second_block=second_block), dtype)
    inside = vol.astype(np.float32) >= np.float32(iso_s)
    assert K.full_tiles(inside) > 0
    r.setQuirks(vra.renderer.QUIRK_DEFAULT)
    r.setMeshWorkspace(0)
    want = reference(complib, ("solid", second_block, np.dtype(dtype).name), vol, iso_s)
    assert want[1]["voxels"].size == 1 + second_block
    for c in range(1, 2 + second_block):                    # whole tiles in every component
        assert K.full_tiles(want[0] == c) > 0
    try:
        r.setComponentIndexBits(index_bits)
        r.setLayout(layout)
        r.setVolume(vol)
        nv, nt = r.extractIsosurface(iso)
        full = r.readMesh()
        assert nt > 0 and M.closed_and_oriented(full[2]) == ""
        assert r.labelComponents(iso) == 1 + second_block
        assert_same_labelling(r, want, "solid with a hole")
        assert r.selectComponents(0, 0) == 1 + second_block
        assert r.extractComponents() == (nv, nt)
        got = r.readMesh()
        assert_same_mesh(got, full, "everything selected")
        assert M.closed_and_oriented(got[2]) == ""
    finally:
        r.setComponentIndexBits(0)
        r.freeMesh()


@WIDTHS
@LAYOUTS
@pytest.mark.parametrize("shape", [(70, 66, 68), (32, 8, 4)], ids=lambda s: "x".join(map(str, s)))
def test_a_volume_that_is_all_inside(vra, complib, handle, shape, layout, index_bits):
    r = handle
    nx, ny, nz = shape
    vol = np.full((nz, ny, nx), K.ON, dtype=np.uint8)
    assert K.full_tiles(vol >= K.ISO) == (nx // 32) * (ny // 8) * (nz // 4) > 0
    want = reference(complib, ("all inside", shape), vol, K.ISO)
    assert want[1]["voxels"].tolist() == [vol.size] and want[1]["first_voxel"].tolist() == [0]
    assert want[1]["bbox"].tolist() == [[0, 0, 0, nx - 1, ny - 1, nz - 1]] and np.all(want[0] == 1)
    try:
        r.setComponentIndexBits(index_bits)
        r.setLayout(layout)
        r.setVolume(vol)
        assert r.labelComponents(K.ISO) == 1
        assert_same_labelling(r, want, "all inside")
        assert r.extractComponents() == (0, 0)              # no edge crosses the surface
    finally:
        r.setComponentIndexBits(0)
        r.freeMesh()
