"""The cases for wavefronts whose lanes part ways in the ray stream's replay loop, without a GPU: every case of
tests/ray_stream_uniform_cases.py reaches the branch it is named for, proven from oracle.render's per-pixel sample counts and
the path model (fast_units) alone."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


U = _load("ray_stream_uniform_cases", ROOT / "tests" / "ray_stream_uniform_cases.py")
C, S = U.C, U.S


def counts(oracle, vol, cam, alpha, window, spacing=(1.0, 1.0, 1.0), mode="grey"):
    n = S.geometric_counts(oracle, vol, U.SIZE, cam, spacing=spacing, window=window)
    spp = oracle.render(vol, S.params(oracle, U.SIZE, cam, alpha, window, mode, spacing=spacing), want_spp=True)[2]
    return n, spp


def test_constants_restate_the_kernel():
    """HELD and UNITS against the kernel's defaults, read as `#define NAME value` whatever the spacing"""
    import re
    text = (ROOT / "volume-renderer_amd" / "csrc" / "vr_stream.hip").read_text()
    value = {k: int(v) for k, v in re.findall(r"^\s*#\s*define\s+(VR_STREAM\w*)\s+(-?\d+)\s*$", text, flags=re.M)}
    assert U.HELD == 2 * value["VR_STREAM_DEPTH"] == 2 * value["VR_STREAM12_DEPTH"]      # K groups composited, K more loaded
    assert value["VR_STREAM_WG"] == 64
    assert U.UNITS == {"packed": 8, "unpacked": 4}


def test_path_model_by_hand():
    """one block of 8 x 8: lanes of n = 20 but one of 13, no opacity -> one fast unit of eight (13 // 8), three of four; the
    same with a lane ended by opacity after 9 samples -> unit 1 of eight fails, unit 2 of four"""
    n = np.full((8, 8), 20, dtype=np.int64)
    n[3, 3] = 13
    assert U.fast_units(n, n, 8)[0][0] == 1 and U.fast_units(n, n, 8)[1][0] == 3
    assert U.fast_units(n, n, 4)[0][0] == 3 and U.fast_units(n, n, 4)[1][0] == 5
    spp = n.copy()
    spp[0, 0] = 9
    assert U.fast_units(n, spp, 8)[0][0] == 1 and U.fast_units(n, spp, 4)[0][0] == 2
    spp[0, 1] = 3
    assert U.fast_units(n, spp, 8)[0][0] == 0 and U.fast_units(n, spp, 4)[0][0] == 0
    n[7, 7] = 0
    assert U.fast_units(n, n, 4)[0][0] == 0


@pytest.mark.parametrize("kind", ["u16", "u8"])
def test_opacity_ends_rays_in_different_units_of_one_wavefront(oracle, kind):
    vol = U.ramp_volume(kind)
    cam = S.pose_block(oracle, U.CLOSE_POSE)
    n, spp = counts(oracle, vol, cam, 1.0, U.ramp_window(kind))
    assert (n > 0).all()                                               # the close pose: every pixel hits
    assert U.scattered_end_blocks(n, spp) >= U.RAMP_MIN_BLOCKS
    for unit in (8, 4):
        fast, total = U.fast_units(n, spp, unit)
        # such a block starts with fast units, leaves them for opacity and has units left after that
        assert np.count_nonzero((fast >= 1) & (fast + 2 <= total)) >= U.RAMP_MIN_BLOCKS, unit


@pytest.mark.parametrize("length", sorted(U.SLAB_Z))
def test_slab_blocks_of_one_ray_length(oracle, length):
    vol = S.residue_volume(oracle, "u16")
    cam = S.pose_block(oracle, U.CLOSE_POSE)
    n, spp = counts(oracle, vol, cam, U.SLAB_ALPHA, (0, 4095), spacing=U.slab_spacing(length))
    assert (n > 0).all() and (spp == n).all()                         # no ray ends by opacity at this alpha
    assert U.equal_blocks(n, length) >= U.SLAB_MIN_BLOCKS
    fast, total = U.fast_units(n, spp, 8)
    ln = U.lanes(n)
    same = (ln.min(axis=1) == length) & (ln.max(axis=1) == length)
    assert (fast[same] == length // 8).all() and (total[same] == (length + 7) // 8).all()
    # n % 8 == 0: every unit of such a block is fast; otherwise exactly the last one is literal
    assert ((total[same] - fast[same]) == (0 if length % 8 == 0 else 1)).all()


def test_slab_lengths_cover_every_residue():
    assert sorted(v % 8 for v in U.SLAB_Z if v < 16) == list(range(8)) and 16 in U.SLAB_Z


def test_mixed_wavefronts(oracle):
    vol = S.residue_volume(oracle, "u16")
    edge = S.pose_block(oracle, U.EDGE_POSE)
    n, spp = counts(oracle, vol, edge, 0.02, (0, 4095))
    assert U.dead_beside_live_blocks(n) >= U.MIXED_MIN_BLOCKS
    ln = U.lanes(n)
    mixed = (ln.min(axis=1) == 0) & (ln.max(axis=1) > 0)
    assert (U.fast_units(n, spp, 8)[0][mixed] == 0).all() and (U.fast_units(n, spp, 4)[0][mixed] == 0).all()
    # the poses of tests/ray_stream_cases.py have no block with exactly one short lane: the rolled camera has
    for pose in S.PARTIAL_POSES:
        assert U.one_short_lane_blocks(S.geometric_counts(oracle, vol, U.SIZE, S.pose_block(oracle, pose), window=(0, 4095))) == 0
    n, spp = counts(oracle, vol, U.rolled_camera(), 0.02, (0, 4095))
    assert U.one_short_lane_blocks(n) >= U.MIXED_MIN_BLOCKS
    srt = np.sort(U.lanes(n), axis=1)
    short = (srt[:, 0] >= 8) & (srt[:, 0] + 8 <= srt[:, 1])
    fast, total = U.fast_units(n, spp, 8)
    # fast up to the short lane's last whole unit, then at least one more unit in which 63 lanes are still whole
    assert (fast[short] == srt[short, 0] // 8).all() and (fast[short] >= 1).all() and (fast[short] + 1 < total[short]).all()


@pytest.mark.parametrize("name,volume,window,mode", U.MODE_CASES, ids=[c[0] for c in U.MODE_CASES])
def test_every_mode_case_has_fast_and_literal_units(oracle, name, volume, window, mode):
    vol = U.mode_volume(oracle, volume)
    cam = S.pose_block(oracle, U.CLOSE_POSE)
    lut = oracle.spline_tf(S.TF_ISO, S.TF_GREY if mode == "grey_tf" else S.TF_COLOUR) if "tf" in mode else None
    n = S.geometric_counts(oracle, vol, U.SIZE, cam, window=(0, 4095))
    assert (n >= 16).all()
    for alpha in U.MODE_ALPHAS:
        spp = oracle.render(vol, S.params(oracle, U.SIZE, cam, alpha, window, mode, lut), want_spp=True)[2]
        for unit in (8, 4):
            fast, total = U.fast_units(n, spp, unit)
            assert np.count_nonzero(fast >= 1) >= 8 and np.count_nonzero(fast < total) >= 8, (alpha, unit)


def test_addressing_cases(oracle):
    vol = S.residue_volume(oracle, "u16")
    n = S.geometric_counts(oracle, vol, U.SIZE, S.pose_block(oracle, U.EDGE_POSE), window=(0, 4095))
    for fmt in ("packed", "unpacked"):
        g = U.block_groups(n, fmt)
        assert np.count_nonzero(g == 1) >= 1, fmt                      # a block of a single group
        assert np.bincount(g[g > 0] % U.HELD, minlength=U.HELD).min() >= 1, fmt      # every residue of the held groups
    assert U.odd_start_blocks(n) >= 8
    # the slab of n = 8: every block is one packed group
    n8 = S.geometric_counts(oracle, vol, U.SIZE, S.pose_block(oracle, U.CLOSE_POSE), spacing=U.slab_spacing(8), window=(0, 4095))
    assert np.count_nonzero(U.block_groups(n8, "packed") == 1) >= U.SLAB_MIN_BLOCKS
