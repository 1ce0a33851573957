"""The cases of tests/test_smoothing_edges_gpu.py reach the parts of csrc/vr_smooth.hip and RendererCore::smoothPasses they are
for -- shown from tests/smoothing_cases.py's restatement of the host rules alone, so that a case which stops reaching its ring,
segment, tile or slab (another shape, another sigma) fails here; that no shape of tests/test_smoothing_gpu.py reaches them,
which is the gap the new file closes; and the CPU definition (tests/smooth_ref/smooth_ref.c) held to an independent numpy
statement of the definition at the large radii, where the GPU file trusts it.  No GPU."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


S = _load("smoothing_cases", HERE / "smoothing_cases.py")
smooth_ref = _load("smooth_ref_binding", HERE / "smooth_ref" / "binding.py")
OLD = _load("old_smoothing_gpu_tests", HERE / "test_smoothing_gpu.py")          # its SHAPES and SIGMAS; nothing of it runs here


@pytest.fixture(scope="module")
def smoothlib(tmp_path_factory):
    return smooth_ref.build(tmp_path_factory.mktemp("smooth_ref_cases"))


def weights_for(vra, sigmas):
    return tuple(vra.smooth_weights(s) if s > 0 else None for s in sigmas)


def every_sigma_used():
    used = set(S.RING_SIGMAS.values()) | set(S.X_SIGMAS) | {1.0} | {s for sig in S.MIXED for s in sig}
    used |= {s for sig, _, _ in S.SLAB_CASES for s in sig} | set(S.THIN_SIGMA) | {S.sweep_sigma(r) for r in range(1, 25)}
    return sorted(s for s in used if s > 0)


# ---------------------------------------------------------------------------------------------------------------
# 1. each case has the property it is named for
# ---------------------------------------------------------------------------------------------------------------
def test_radius_is_the_librarys_weight_count(vra):
    for sigma in every_sigma_used():
        assert vra.smooth_weights(sigma).size == 2 * S.radius(sigma) + 1, sigma
    assert {r: S.radius(s) for r, s in S.RING_SIGMAS.items()} == {8: 8, 9: 9, 24: 24}
    assert [S.radius(S.sweep_sigma(r)) for r in range(1, 25)] == list(range(1, 25))
    assert S.radius(0.5) == 2 and S.radius(1.0) == 3


def test_the_named_radii_sit_at_the_limits_of_the_two_rings():
    assert S.col_plan(10, 6, 200, 8).ring == 32 and 16 + 2 * 8 == 32            # full
    assert S.col_plan(10, 6, 200, 9).ring == 64                                 # the first radius of the large ring
    assert S.col_plan(10, 6, 200, 24).ring == 64 and 16 + 2 * 24 == 64          # full
    assert [S.col_plan(37, 33, 35, r).ring for r in range(1, 25)] == [32] * 8 + [64] * 16


@pytest.mark.parametrize("name", list(S.COLUMN_PLANS))
def test_column_shapes_have_interior_segments_and_a_short_last_one(name):
    nx, ny, nz = S.SHAPES[name]
    want_y, want_z = S.COLUMN_PLANS[name]
    for r in S.RING_SIGMAS:
        plans = []
        if want_y:
            p = S.col_plan(nx, nz, ny, r)
            assert p[1:] == want_y
            plans.append(p)
        if want_z:
            p = S.col_plan(nx, ny, nz, r)
            assert p[1:] == want_z
            plans.append(p)
        for p in plans:
            assert p.segs >= 4 and 0 < p.last < S.STEP                          # seams on both sides; a last segment below a step
            assert p.seg <= 64                                                  # ... and the split stopped there, not at 2048 workgroups
            # 2. the ring wraps: a whole segment has a step whose new rows overwrite the oldest ones
            assert p.steps > S.first_wrapping_step(r, p.ring)
    assert any(v[0] and v[0][2] >= 4 for v in S.COLUMN_PLANS.values())          # a segment of 64 outputs: four steps
    assert any(v[1] and v[1][2] >= 4 for v in S.COLUMN_PLANS.values())


def test_where_the_ring_wraps():
    """from the second step at the radii that fill a ring; only from the third at r = 9 -- why its column cases need three steps"""
    assert S.first_wrapping_step(8, 32) == 1 and S.first_wrapping_step(24, 64) == 1 and S.first_wrapping_step(9, 64) == 2
    assert S.first_wrapping_step(1, 32) == 1 and S.first_wrapping_step(7, 32) == 1 and S.first_wrapping_step(16, 64) == 2


def test_the_split_of_both_stops_at_the_segment_floor():
    nx, ny, nz = S.SHAPES["BOTH"]
    assert -(-nx // 64) * -(-nz // 4) == 38 and 38 * 4 < S.MIN_WORKGROUPS


def test_sweep_runs_every_radius_in_one_segment_of_several_steps():
    nx, ny, nz = S.SHAPES["SWEEP"]
    for r in range(1, 25):
        for p in (S.col_plan(nx, nz, ny, r), S.col_plan(nx, ny, nz, r)):
            assert p.segs == 1 and p.steps == 3
    assert S.x_tiles(nx) == 1 and nx % 4 == 1


def test_x_shapes():
    assert S.x_tiles(261) == 3 and 261 - 2 * S.X_TILE == 5 and 261 % 4 == 1     # 128 + 128 + 5; a last quad of one voxel
    assert S.SHAPES["XT"][1] % 4 and S.SHAPES["XT"][2] % 4
    assert S.SHAPES["XT"][0] % 4 != 0                                            # rows of the linear layout start unaligned
    assert S.x_tiles(256) == 2 and 256 % S.X_TILE == 0
    assert S.x_tiles(129) == 2 and 129 - S.X_TILE == 1
    assert all(S.x_tiles(shape[0]) == 1 for name, shape in S.SHAPES.items() if not name.startswith("XT"))
    assert sorted(S.radius(s) for s in S.X_SIGMAS) == [2, 8, 24]
    # the seam columns are exactly the voxels within 24 of x = 128 and x = 256
    a, b = S.XT_SEAM_COLUMNS
    assert (a.start, a.stop, b.start, b.stop) == (128 - 24, 128 + 24, 256 - 24, 261)


def test_slab_cases():
    nx, ny, nz = S.SHAPES["BOTH"]
    for sig, planes, slab in S.SLAB_CASES:
        rz = S.radius(sig[2]) if sig[2] > 0 else 0
        plan = S.slab_plan(nx, ny, nz, rz, S.workspace_bytes(S.SHAPES["BOTH"], planes))
        assert plan == S.SlabPlan(planes, slab), (sig, planes)
        ranges = S.slab_ranges(nz, rz, slab)
        assert len(ranges) == -(-nz // slab) and all(e1 - e0 <= planes for _, _, e0, e1 in ranges)
        if sig[1] > 0:                                                          # the y pass runs its four segments inside every slab
            assert all(S.col_plan(nx, e1 - e0, ny, S.radius(sig[1])).segs == 4 for _, _, e0, e1 in ranges)
    slabs = {(sig, planes): slab for sig, planes, slab in S.SLAB_CASES}
    assert slabs[((8.0, 8.0, 8.0), 49)] == 1 and 49 == 2 * 24 + 1                # the smallest workspace the call accepts
    assert S.slab_plan(nx, ny, nz, 24, S.workspace_bytes(S.SHAPES["BOTH"], 48)) is None
    assert slabs[((8.0, 8.0, 8.0), 65)] % S.STEP == 1                            # seams inside 16-row steps
    assert len(S.instances((0.0, 8.0, 8.0))) - 1 == 1 and ("y", "v", "f") in S.instances((0.0, 8.0, 8.0))      # one buffer, written by y
    assert S.instances((8.0, 3.0, 0.0)) == {("x", "v", "f"), ("y", "f", "v")}


def test_thin_is_shorter_than_one_slab_of_the_largest_radius():
    nx, ny, nz = S.SHAPES["THIN"]
    rz = S.radius(S.THIN_SIGMA[2])
    assert rz == 24 and nz < 2 * rz + 1
    assert S.slab_plan(nx, ny, nz, rz, S.workspace_bytes(S.SHAPES["THIN"], S.THIN_PLANES_OK)) == S.SlabPlan(nz, nz)     # one piece
    assert S.slab_plan(nx, ny, nz, rz, S.workspace_bytes(S.SHAPES["THIN"], S.THIN_PLANES_REFUSED)) is None


def test_the_subsets_select_every_kernel_instance():
    for R in S.RING_SIGMAS.values():
        subsets = S.SUBSETS(R)
        assert len(subsets) == len(set(subsets)) == 7 and all(set(sig) <= {0.0, R} for sig in subsets)
        assert set().union(*(S.instances(sig) for sig in subsets)) == S.ALL_INSTANCES
    assert S.instances((8.0, 0.0, 0.0)) == {("x", "v", "v")}
    assert S.instances((8.0, 8.0, 8.0)) == {("x", "v", "f"), ("y", "f", "f"), ("z", "f", "v")}
    assert S.instances((0.0, 8.0, 8.0)) == {("y", "v", "f"), ("z", "f", "v")}
    # MIXED: each named radius once on each axis
    assert [sorted(S.radius(s) for s in sig) for sig in S.MIXED] == [[8, 9, 24]] * 3
    assert [{S.radius(sig[a]) for sig in S.MIXED} for a in range(3)] == [{8, 9, 24}] * 3


# ---------------------------------------------------------------------------------------------------------------
# 3. no earlier GPU shape has these properties
# ---------------------------------------------------------------------------------------------------------------
def old_column_passes():
    """(axis, instance, radius, plan) of every column pass tests/test_smoothing_gpu.py runs bit-exactly over SHAPES x SIGMAS (its
    full-range and slab tests included: the same sigmas on 33 x 32 x 31 and on 70 x 66 x 68 in slabs)"""
    out = []
    shapes = [(s, None) for s in OLD.SHAPES] + [((33, 32, 31), None)]
    runs = [(shape, sig, None) for shape, _ in shapes for sig in OLD.SIGMAS]
    runs += [((70, 66, 68), sig, planes) for sig, planes in (((1.0, 1.0, 1.0), 11), ((0.0, 2.0, 3.0), 19), ((0.5, 2.0, 0.0), 5), ((8.0, 0.3, 1.0), 7))]
    for (nx, ny, nz), sig, planes in runs:
        rz = S.radius(sig[2]) if sig[2] > 0 else 0
        if planes is None:
            ranges = [(0, nz, 0, nz)]
        else:
            plan = S.slab_plan(nx, ny, nz, rz, planes * nx * ny * 4 + 17)
            ranges = S.slab_ranges(nz, rz, plan.slab)
        for s0, s1, e0, e1 in ranges:
            for inst in S.instances(sig):
                if inst[0] == "y":
                    last = sig[2] == 0
                    nb = (s1 - s0) if last else (e1 - e0)
                    out.append(("y", inst, S.radius(sig[1]), S.col_plan(nx, nb, ny, S.radius(sig[1]))))
                elif inst[0] == "z":
                    out.append(("z", inst, rz, S.col_plan(nx, ny, s1 - s0, rz)))
    return out


def test_no_earlier_shape_reaches_the_large_ring_on_y_or_with_fp32_input():
    passes = old_column_passes()
    assert passes and any(p[0] == "y" for p in passes) and any(p[0] == "z" for p in passes)
    assert not [p for p in passes if p[0] == "y" and p[3].ring == 64]
    big = [p for p in passes if p[3].ring == 64]
    assert big and all(p[0] == "z" and p[2] == 9 for p in big)                  # z at r = 9, nothing else
    # ... as the single-pass instance, or fed fp32 planes by the slab test's (0, 2, 3) at 19 planes: slabs of ONE output plane,
    # a single step, so with fp32 input the large ring never wrapped (r = 9 wraps at the third step)
    assert {p[1] for p in big} == {("z", "v", "v"), ("z", "f", "v")}
    assert all(p[3].steps == 1 and p[3].last == 1 for p in big if p[1] == ("z", "f", "v"))
    assert not [p for p in passes if p[2] in (8, 24)]                           # neither ring was ever full on a column pass


def test_no_earlier_column_has_an_interior_segment_a_fourth_step_or_a_short_last_segment():
    passes = old_column_passes()
    assert max(p[3].segs for p in passes) == 2                                  # a seam on one side at the most
    assert max(p[3].steps for p in passes) < 4                                  # no segment of 64 outputs
    assert not [p for p in passes if p[3].segs > 1 and p[3].last < S.STEP]


def test_no_earlier_bit_exact_x_pass_has_a_second_tile():
    assert max(S.x_tiles(nx) for nx, _, _ in list(OLD.SHAPES) + [(33, 32, 31), (41, 39, 40), (24, 20, 22)]) == 1
    assert {S.radius(sig[0]) for sig in OLD.SIGMAS if sig[0] > 0} == {2, 3, 24}
    assert {S.radius(sig[1]) for sig in OLD.SIGMAS if sig[1] > 0} == {1, 3, 6}
    assert {S.radius(sig[2]) for sig in OLD.SIGMAS if sig[2] > 0} == {3, 9}


# ---------------------------------------------------------------------------------------------------------------
# 4. the reference at the new radii against an independent statement of the definition
# ---------------------------------------------------------------------------------------------------------------
def numpy_smooth(vol, weights):
    """the definition in numpy: per pass acc = 0, then acc = acc + w_t * in[clip(i + t)] for t = -r .. r in this order, every
    product and every sum one fp32 operation on whole arrays; x, then y, then z; rint (half to even), clipped to the type"""
    a = vol.astype(np.float32)
    ran = False
    for axis, w in zip((2, 1, 0), weights):                                     # x is the last index of [z, y, x]
        if w is None:
            continue
        assert w.dtype == np.float32
        r = (w.size - 1) // 2
        n = a.shape[axis]
        acc = np.zeros_like(a)
        for t in range(-r, r + 1):
            prod = w[t + r] * np.take(a, np.clip(np.arange(n) + t, 0, n - 1), axis=axis)
            assert prod.dtype == np.float32
            acc = acc + prod
        a, ran = acc, True
    if not ran:
        return vol.copy()
    return np.clip(np.rint(a), 0, S.peak(vol.dtype)).astype(vol.dtype)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
@pytest.mark.parametrize("name", list(S.SHAPES))
def test_the_reference_equals_the_numpy_statement_at_the_new_radii(vra, smoothlib, name, dtype):
    vol = S.random_volume(name, dtype)
    for sig in S.SUBSETS(8.0) + S.MIXED:
        w = weights_for(vra, sig)
        got, want = smooth_ref.smooth(smoothlib, vol, w), numpy_smooth(vol, w)
        assert np.array_equal(got, want), f"{name} {np.dtype(dtype).name} sigma {sig}: {int(np.sum(got != want))} voxels differ"
    assert not np.array_equal(got, vol)


def test_the_value_volumes_are_what_they_are_named():
    nx, ny, nz = S.SHAPES["BOTH"]
    for dtype in (np.uint8, np.uint16):
        hi = S.peak(dtype)
        c = S.value_volume("checkerboard", dtype)
        assert c.shape == (nz, ny, nx) and c.dtype == dtype and set(np.unique(c)) == {0, hi}
        assert np.all(c[:, :, 1:] != c[:, :, :-1]) and np.all(c[:, 1:] != c[:, :-1]) and np.all(c[1:] != c[:-1])
        k = S.value_volume("corners", dtype)
        assert int(np.sum(k == 0)) == 8 and int(np.sum(k == hi)) == k.size - 8 and k[0, 0, 0] == 0 and k[-1, -1, -1] == 0 and k[0, -1, 0] == 0
        for kind, at in (("centre", (nz // 2, ny // 2, nx // 2)), ("origin", (0, 0, 0))):
            v = S.value_volume(kind, dtype)
            assert v[at] == hi and int(np.count_nonzero(v)) == 1
