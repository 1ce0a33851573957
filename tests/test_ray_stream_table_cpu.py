"""The cases of the ray stream's hybrid classification, without a GPU: every case of tests/ray_stream_table_cases.py reaches what
it is named for -- proven from oracle.render's per-pixel sample counts and the volumes alone -- and no shape of the older stream
tests reaches the hybrid at all."""
import importlib.util
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


T = _load("ray_stream_table_cases", ROOT / "tests" / "ray_stream_table_cases.py")
U, C, S = T.U, T.C, T.S
CSRC = ROOT / "volume-renderer_amd" / "csrc"
TABLE = T.POSITIONS[T.SHARE]
ARITH = tuple(u for u in range(S.G) if u not in TABLE)


def test_constants_restate_the_sources():
    text = (CSRC / "vr_stream.hip").read_text()
    value = {k: int(v) for k, v in re.findall(r"^\s*#\s*define\s+(VR_STREAM\w*)\s+(-?\d+)\s*$", text, flags=re.M)}
    assert value["VR_STREAM_TSHARE"] == T.SHARE and value["VR_STREAM_TWG"] == T.TABLE_WG
    # table_pos of the kernel: every fourth, every second or every sample
    assert "TSHARE == 4 || (TSHARE == 2 && (u & 1) != 0) || (TSHARE == 1 && u == 3)" in text
    assert T.POSITIONS == {1: (3,), 2: (1, 3), 4: (0, 1, 2, 3)}
    head = (CSRC / "vr_stream.h").read_text()
    assert re.search(r"kStreamTableMax\s*=\s*4096\b", head) and T.TABLE_MAX == 4096
    assert re.search(r"kStreamTableMinBytes\s*=\s*256ull\s*<<\s*20\b", head) and T.TABLE_MIN_BYTES == 256 << 20
    assert re.search(r"FAST_LUT_MAX\s*=\s*4096\b", (CSRC / "vr_device.h").read_text())
    if T.SHARE < 4:
        assert TABLE and ARITH


def test_eligibility_by_hand():
    assert T.eligible((0, 4095), "grey", True) and T.eligible((0, 4095), "mip", False)
    assert not T.eligible((0, 4096), "grey", False)                     # one entry more than the table holds
    assert not T.eligible((0, 4095), "grey_tf", False) and not T.eligible((0, 4095), "tf", True)
    far = (-(1 << 24), -(1 << 24) + 100)                                 # a narrow window beyond the bound of the shifted constants
    assert T.eligible(far, "grey", False) and not T.eligible(far, "grey", True, 1000)
    for name, volume, window, mode, packed, unpacked in T.CASES:
        base = T.OFFSET_BASE if volume == "offset" else 0
        assert (T.eligible(window, mode, True, base), T.eligible(window, mode, False)) == (packed, unpacked), name


def test_the_volumes_have_the_ranges_the_cases_assume(oracle):
    vol = T.extremes_volume(oracle)
    assert (int(vol.min()), int(vol.max())) == (0, 4095)                 # a span of exactly 4095: the packed format holds it
    off = T.offset_extremes_volume(oracle)
    assert (int(off.min()), int(off.max())) == (T.OFFSET_BASE, T.OFFSET_BASE + 4095)
    windows = {name: (volume, window) for name, volume, window, *_ in T.CASES}
    assert windows["window_is_the_range"][1] == (0, 4095) and windows["offset_window_is_the_range"][1] == (1000, 5095)
    assert windows["window_is_the_range"][1][1] - windows["window_is_the_range"][1][0] + 1 == T.TABLE_MAX
    assert windows["one_entry_more"][1][1] - windows["one_entry_more"][1][0] + 1 == T.TABLE_MAX + 1
    assert windows["beyond_2_24"][1][1] >= 1 << 24


@pytest.mark.parametrize("volume,window", [("extremes", (1000, 3000)), ("offset", (2000, 4000))], ids=["extremes", "offset"])
def test_clamped_samples_land_at_table_and_arithmetic_positions(oracle, volume, window):
    """samples below the window and samples above it are the FIRST such sample of at least MIN_RAYS rays at every position of a
    group of four (and of eight: the packed group), from the close pose; the first such sample inside a slab of the volume, slab
    by slab (slab_residues)"""
    vol = T.volume(oracle, volume)
    cam = S.pose_block(oracle, T.CLOSE_POSE)
    for mask in (vol < window[0], vol > window[1]):
        by_eight = T.slab_residues(oracle, mask, cam, 8)
        assert by_eight.min() >= T.MIN_RAYS, by_eight
        by_four = by_eight[:4] + by_eight[4:]
        assert min(by_four[u] for u in TABLE) >= T.MIN_RAYS and min(by_four[u] for u in ARITH or TABLE) >= T.MIN_RAYS


@pytest.mark.parametrize("volume,window", [("extremes", (0, 4095)), ("extremes", (1000, 3000)), ("offset", (1000, 5095)), ("offset", (2000, 4000))],
                         ids=["range", "inside", "offset_range", "offset_inside"])
def test_the_first_and_the_last_entry_are_read(oracle, volume, window):
    """voxels of exactly the window's first and last value are sampled, at table positions and at arithmetic ones"""
    vol = T.volume(oracle, volume)
    cam = S.pose_block(oracle, T.CLOSE_POSE)
    for value in window:
        assert np.count_nonzero(vol == value) > 0, value
        by_four = T.slab_residues(oracle, vol == value, cam, S.G)
        assert min(by_four[u] for u in TABLE) >= 1 and min(by_four[u] for u in ARITH or TABLE) >= 1, (value, by_four)


def test_rays_end_by_opacity_at_every_position(oracle):
    vol = S.residue_volume(oracle, "u16")
    covered = np.zeros(8, dtype=np.int64)
    for pose, cam in S.residue_cameras(oracle):
        n = S.geometric_counts(oracle, vol, T.SIZE, cam, window=(0, 4095))
        for alpha in (1.0, 0.3):
            out = oracle.render(vol, S.params(oracle, T.SIZE, cam, alpha, (0, 4095)), want_spp=True)
            spp = out[2].astype(np.int64)
            early = (n > 0) & (spp < n)
            covered += np.bincount(spp[early] % 8, minlength=8)
    assert covered.min() >= T.MIN_RAYS                                   # the first sample left out sits at every position of a group of 8


def test_dead_lanes_and_empty_workgroups(oracle):
    vol = T.extremes_volume(oracle)
    edge = S.geometric_counts(oracle, vol, T.SIZE, S.pose_block(oracle, T.EDGE_POSE), window=(0, 4095))
    assert U.dead_beside_live_blocks(edge) >= U.MIXED_MIN_BLOCKS
    front = S.geometric_counts(oracle, vol, T.SIZE, S.pose_block(oracle, T.FAR_POSE), window=(0, 4095))
    for threads in (512, 256):
        empty, live = T.empty_workgroups(front, threads)
        assert empty >= 2 and live >= 2, threads                         # workgroups that build no table beside ones that do


def test_the_older_stream_tests_never_reach_the_hybrid():
    """they never set the table mode, and under the default mode the hybrid needs a stream of more than TABLE_MIN_BYTES: their
    largest image is 600 x 456, no ray through the unit box of a 64^3 volume has 200 samples (sqrt(3) / step), and the step-cap
    case has 96 x 64 rays of at most MAX_STEPS one-byte samples"""
    for f in ("test_ray_stream_gpu.py", "test_ray_stream_edges_gpu.py", "test_ray_stream_pack_gpu.py", "test_ray_stream_uniform_gpu.py"):
        assert "RayStreamTable" not in (ROOT / "tests" / f).read_text(), f
    largest = max(w * h for w, h in list(S.SCAN_SIZES) + S.PARTIAL_SIZES + [S.RESIDUE_SIZE, S.REFUSAL_SIZE, S.ANISO_SIZE])
    assert largest == 600 * 456
    # (every lane of every block padded to 200 samples in whole groups of 8, two bytes each)
    assert S.stream_grid(600, 456).blocks * 64 * 208 * 2 < T.TABLE_MIN_BYTES
    assert S.CAP_SIZE[0] * S.CAP_SIZE[1] * (S.MAX_STEPS + 8) < T.TABLE_MIN_BYTES
