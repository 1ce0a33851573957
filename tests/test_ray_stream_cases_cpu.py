"""The cases of tests/test_ray_stream_edges_gpu.py reach the branches of csrc/vr_stream.hip they are for -- shown from the CPU
oracle and from tests/ray_stream_cases.py's restatement of the host arithmetic alone, so that a case which stops reaching its
branch (another volume, another pose, another image size) fails here.  No GPU."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

_spec = importlib.util.spec_from_file_location("ray_stream_cases", Path(__file__).resolve().parent / "ray_stream_cases.py")
S = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(S)


@pytest.mark.parametrize("size", list(S.SCAN_SIZES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_scan_sizes(size):
    """block count, blocks per scan thread, the first thread with an empty range and the thread `blocks` cuts short"""
    blocks, per, idle, cut = S.SCAN_SIZES[size]
    g = S.stream_grid(*size)
    assert g.blocks == blocks and g.blocks_x % 4 == 0 and g.blocks_y % 2 == 0
    assert S.scan_shape(blocks) == S.Scan(per, idle, cut)


def test_scan_sizes_cover_the_serial_run():
    pers = sorted(v[1] for v in S.SCAN_SIZES.values())
    assert pers[0] == 1 and 2 in pers and 3 in pers and pers[-1] >= 4
    assert S.SCAN_SIZES[(256, 256)][0] == S.SCAN_THREADS                       # the boundary itself
    assert any(v[2] is not None and v[3] is None for v in S.SCAN_SIZES.values())     # idle threads after whole runs
    assert sum(v[3] is not None for v in S.SCAN_SIZES.values()) >= 2           # a cut-short thread, at two values of per


def test_scan_restatement_on_small_counts():
    assert S.scan_shape(1) == S.Scan(1, 1, None)
    assert S.scan_shape(1025) == S.Scan(2, 513, 512)
    assert S.scan_shape(2048) == S.Scan(2, None, None)


def test_partial_sizes_cut_blocks():
    """101x77 and 97x65 have blocks with lanes on both sides of the image edge, along x, along y and at the corner, and whole
    blocks outside (the padding to 32x16 tiles); under kQuirkTruncGrid the limits 96 / 64 are multiples of 8: no block is cut,
    more are empty; 8x8 is one whole block and seven empty ones, and nothing at all under the quirk"""
    assert S.cut_blocks((101, 77)) == (22, 30) and S.cut_blocks((97, 65)) == (21, 43)
    assert S.cut_blocks((101, 77), True) == (0, 64) and S.cut_blocks((97, 65), True) == (0, 64)
    assert S.cut_blocks((8, 8)) == (0, 7) and S.cut_blocks((8, 8), True) == (0, 8)
    assert 97 % 8 == 1 and 65 % 8 == 1                                         # one column and one row into a new block
    # the row range and the stripes begin or end inside a block
    rows = S.local_rows(77, row_range=S.PARTIAL_ROW_RANGE)
    assert rows[0] % 8 != 0 and len(rows) % 8 != 0 and -1 not in rows
    rows = S.local_rows(77, stripes=S.PARTIAL_STRIPES)
    assert rows == list(range(16, 32)) + list(range(64, 77)) + [-1] * 3


@pytest.mark.parametrize("size", [(101, 77), (97, 65)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_cut_blocks_hold_rays_from_the_close_pose(oracle, size):
    """from the close pose every pixel's ray has samples, and so has the ray of every lane beyond the image's edge (the same
    camera on the image padded to whole blocks, shifted so that the pixels coincide, is not needed: a ray through a pixel centre
    outside the image is still a ray of the camera) -- here: all pixels of the last column and the last row hit the box; from the
    default camera none of them does"""
    vol = S.residue_volume(oracle, "u8")
    n = S.geometric_counts(oracle, vol, size, S.pose_block(oracle, S.CLOSE_POSE))
    assert n.min() > 0
    assert len(np.unique(S.block_groups(S.local_counts(n, S.local_rows(size[1]))))) >= 4      # blocks of several lengths
    n = S.geometric_counts(oracle, vol, size, S.pose_block(oracle, ()))
    assert not n[:, -1].any() and not n[-1, :].any()


def test_local_rows_restatement():
    assert S.local_rows(5) == [0, 1, 2, 3, 4]
    assert S.local_rows(40, trunc=True) == list(range(32)) + [-1] * 8
    assert S.local_rows(40, stripes=(16, 2, 3)) == list(range(32, 40)) + [-1] * 8
    assert S.local_rows(40, stripes=(16, 0, 2)) == list(range(16)) + list(range(32, 40)) + [-1] * 8
    n = S.local_counts(np.arange(12).reshape(3, 4) + 1, [2, -1, 0])
    assert n.tolist() == [[9, 10, 11, 12], [0, 0, 0, 0], [1, 2, 3, 4]]
    n = S.local_counts(np.ones((3, 20), dtype=int), [0, 1, 2], trunc=True)
    assert n[:, :16].all() and not n[:, 16:].any()


def test_stream_size_model_by_hand():
    """9 x 17 pixels: 4 x 4 blocks of which the first two rows and columns hold pixels.  Block (0, 0) has a longest ray of 5
    samples (2 groups), block (1, 0) one of 4 (1 group), block (0, 1) one of 1 (1 group), block (0, 2) -- the 17th row -- one of
    9 (3 groups); the rest are empty"""
    n = np.zeros((17, 9), dtype=np.int64)
    n[3, 2] = 5; n[7, 7] = 3
    n[0, 8] = 4
    n[8, 0] = 1
    n[16, 1] = 9
    groups = S.block_groups(n)
    assert groups.shape == (4, 4)
    want = np.zeros((4, 4), dtype=np.int64)
    want[0, 0], want[0, 1], want[1, 0], want[2, 0] = 2, 1, 1, 3
    assert np.array_equal(groups, want)
    for b in (1, 2):
        assert S.stream_bytes(n, b) == 7 * 256 * b + 16 + 16 * 64 * 2 + 17 * 8
    assert S.stream_bytes(np.zeros((8, 8), dtype=np.int64), 1) == 16 + 8 * 128 + 9 * 8     # no sample at all: the slack and the small arrays


def test_step_cap_case(oracle):
    """rays down the 16384-voxel axis stop at 10000 samples with dest.a far below 0.95; others leave the box earlier"""
    vol = S.cap_volume()
    p = S.params(oracle, S.CAP_SIZE, S.cap_camera(), S.CAP_ALPHA, S.CAP_WINDOW, spacing=S.CAP_SPACING)
    frame, _, spp = oracle.render(vol, p, want_spp=True)
    assert np.count_nonzero(spp == S.MAX_STEPS) >= 100
    assert np.count_nonzero((spp > 0) & (spp < S.MAX_STEPS)) >= 100
    assert spp.max() == S.MAX_STEPS and frame[..., 3].max() < 0.5
    n = S.geometric_counts(oracle, vol, S.CAP_SIZE, S.cap_camera(), spacing=S.CAP_SPACING)
    assert np.array_equal(n, spp)                                              # no ray of the frame ends by opacity


@pytest.mark.parametrize("kind", ["u8", "u16"])
def test_residue_frames_end_rays_at_every_residue(oracle, kind):
    vol = S.residue_volume(oracle, kind)
    win = S.residue_window(kind)
    for pose, cam in S.residue_cameras(oracle):
        n = S.geometric_counts(oracle, vol, S.RESIDUE_SIZE, cam, window=win)
        for alpha in S.RESIDUE_ALPHAS:
            frame, _, spp = oracle.render(vol, S.params(oracle, S.RESIDUE_SIZE, cam, alpha, win), want_spp=True)
            early, geometric, groups = S.residue_bins(spp, frame[..., 3], n)
            what = (kind, pose, alpha, early.tolist(), geometric.tolist(), groups.tolist())
            assert geometric.min() >= S.RESIDUE_MIN_RAYS and groups.min() >= S.RESIDUE_MIN_RAYS, what
            if alpha == 0.004:
                assert early.sum() == 0, what                                  # every ray crosses the volume
            else:
                assert early.min() >= S.RESIDUE_MIN_RAYS, what
        blocks = S.block_groups(S.local_counts(n, S.local_rows(S.RESIDUE_SIZE[1])))
        by_residue = np.bincount(blocks[blocks > 0] % S.DEPTH, minlength=S.DEPTH)
        if not pose:
            assert np.count_nonzero(by_residue) == 1                           # why the second pose is there
        else:
            assert by_residue.min() >= S.RESIDUE_MIN_BLOCKS, (kind, pose, by_residue.tolist())


@pytest.mark.parametrize("kind", ["u8", "u16"])
@pytest.mark.parametrize("value,alpha,count", S.CONSTANT_CASES)
def test_constant_volumes_end_every_long_ray_at_one_index(oracle, kind, value, alpha, count):
    """every ray with more than `count` samples in the box ends after exactly `count`: 11 = 4 * 2 + 3 -- the last sample of a
    group is the first one left out, what the whole-group shortcut's test decides -- and 12 = 4 * 3"""
    assert [c % S.G for _, _, c in S.CONSTANT_CASES] == [3, 0]
    vol = S.constant_volume(value, kind)
    cam = oracle.default_camera_block()
    n = S.geometric_counts(oracle, vol, S.RESIDUE_SIZE, cam)
    frame, _, spp = oracle.render(vol, S.params(oracle, S.RESIDUE_SIZE, cam, alpha, (0, 255)), want_spp=True)
    long_rays = n > count
    assert np.count_nonzero(long_rays) >= 1000 and (spp[long_rays] == count).all()
    assert (frame[..., 3][long_rays] >= S.END_ALPHA).all()
    short = (n > 0) & ~long_rays
    assert np.count_nonzero(short) >= 100 and np.array_equal(spp[short], n[short])     # the box's corners: shorter rays end geometrically


@pytest.mark.parametrize("kind", ["u8", "u16"])
def test_refusal_views(oracle, kind):
    """the close view's stream is more than twice the far view's, by the size model"""
    vol = S.residue_volume(oracle, kind)
    sizes = []
    for cam in S.refusal_cameras(oracle):
        n = S.geometric_counts(oracle, vol, S.REFUSAL_SIZE, cam, window=S.residue_window(kind))
        sizes.append(S.stream_bytes(S.local_counts(n, S.local_rows(S.REFUSAL_SIZE[1])), vol.dtype.itemsize))
    assert sizes[0] >= 2 * sizes[1] + 8192, sizes


def test_inside_camera_and_spacing(oracle):
    """the eye of B7's camera block lies inside the anisotropic box, and most of its rays start there; every orbit pose hits"""
    half = S.box_half(S.ANISO_DIMS, S.ANISO_SPACING)
    assert (np.abs(np.array(S.INSIDE_EYE)) < half * 0.9).all()
    assert len(set(np.round(half, 6))) == 3                                    # three different extents, none of them 0.5
    vol = S.aniso_volume("u8")
    n = S.geometric_counts(oracle, vol, S.ANISO_SIZE, S.inside_camera(), spacing=S.ANISO_SPACING)
    assert np.count_nonzero(n) == n.size                                       # from inside every ray hits
    for name, cam in S.orbit_blocks(oracle):
        n = S.geometric_counts(oracle, vol, S.ANISO_SIZE, cam, spacing=S.ANISO_SPACING)
        assert np.count_nonzero(n) >= 1000 and np.count_nonzero(n == 0) >= 1000, name
