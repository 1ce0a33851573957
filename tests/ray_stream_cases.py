"""TEST INFRASTRUCTURE ONLY -- the edges of the ray-ordered sample stream (csrc/vr_stream.hip), for
tests/test_ray_stream_cases_cpu.py and tests/test_ray_stream_edges_gpu.py.

The stream's kernels have branches that depend on the image size (how many 8x8 stream blocks there are, whether the scan gives a
thread more than one block, whether a block is cut by the image edge), on where a ray ends (leaving the box, dest.a >= 0.95, the
step cap; which sample of a group of four) and on the volume (32-bit or 64-bit offsets in the record pass).  This module restates
the host-side arithmetic that decides them -- streamGrid, the scan's blocks per thread, the launch's local rows, the stream's size
-- and holds the cases.  The CPU file proves from the oracle alone that each case reaches its branch; the GPU file renders them.

Volumes are indexed [z, y, x]; dims are (nx, ny, nz); sizes are (width, height).
"""
from collections import namedtuple

import numpy as np

STREAM = "raymarch_stream_kernel"
G = 4                                   # kStreamGroup: samples a lane reads with one load
DEPTH = 4                               # VR_STREAM_DEPTH: groups a lane keeps in flight
TILE_W, TILE_H = 32, 16                 # kFastTileW x kFastTileH: the replay kernel's workgroup tile, 4 x 2 stream blocks
SCAN_THREADS = 1024                     # stream_scan_kernel: one workgroup
MAX_STEPS = 10000
LOCAL_SIZE = 16                         # kLocalSize: kQuirkTruncGrid cuts the image to whole 16 x 16 groups
END_ALPHA = 0.95                        # dest.a >= 0.95 -> break (VolumeRenderer.cs:118)

TF_ISO = [0, 60, 140, 255]
TF_COLOUR = [[0.0, 0.0, 0.0, 0.0], [1.0, 0.2, 0.1, 0.1], [0.2, 1.0, 0.3, 0.6], [1.0, 1.0, 1.0, 1.0]]
TF_GREY = [[0.0, 0.0, 0.0, 0.0], [0.3, 0.3, 0.3, 0.1], [0.7, 0.7, 0.7, 0.6], [1.0, 1.0, 1.0, 1.0]]
MODES = ("grey", "mip", "tf", "mip_tf", "grey_tf")


# ---------------------------------------------------------------------------------------------------------------
# the host's arithmetic, restated
# ---------------------------------------------------------------------------------------------------------------
Grid = namedtuple("Grid", "blocks_x blocks_y blocks")
Scan = namedtuple("Scan", "per first_idle cut_short")     # threads by index; None: there is none


def stream_grid(width, rows):
    """streamGrid (csrc/vr_stream.h): whole 32 x 16 tiles of 8 x 8 blocks over the launch's local rows"""
    bx = (width + TILE_W - 1) // TILE_W * (TILE_W // 8)
    by = (rows + TILE_H - 1) // TILE_H * (TILE_H // 8)
    return Grid(bx, by, bx * by)


def scan_shape(blocks):
    """stream_scan_kernel's partition: thread t sums blocks [min(t * per, blocks), min(t * per + per, blocks)).  first_idle: the
    first thread whose range is empty; cut_short: the thread whose range `blocks` ends before its per-th block"""
    per = (blocks + SCAN_THREADS - 1) // SCAN_THREADS
    first_idle = cut = None
    for t in range(SCAN_THREADS):
        b0 = min(t * per, blocks)
        b1 = min(b0 + per, blocks)
        if b0 == b1 and first_idle is None:
            first_idle = t
        if 0 < b1 - b0 < per:
            cut = t
    return Scan(per, first_idle, cut)


def local_rows(height, row_range=None, stripes=None, trunc=False):
    """The image row of every local row of a launch (launch_local_rows and the kernels' row mapping), -1 where the local row
    holds no pixel (beyond the image, the range or kQuirkTruncGrid's limit).  row_range: (begin, end); stripes: (rows, index,
    count) -- one or neither."""
    row_lim = height // LOCAL_SIZE * LOCAL_SIZE if trunc else height
    if stripes is not None:
        srows, index, count = stripes
        total = (height + srows - 1) // srows
        mine = (total - index + count - 1) // count
        rows = [((ly // srows) * count + index) * srows + ly % srows for ly in range(mine * srows)]
        end = height
    else:
        begin, end = (0, height) if row_range is None else row_range
        rows = list(range(begin, end))
    return [py if py < end and py < row_lim else -1 for py in rows]


def local_counts(spp, rows, trunc=False):
    """the per-pixel counts of a full-frame array over the launch's local rows; 0 where there is no pixel"""
    h, w = spp.shape
    col_lim = w // LOCAL_SIZE * LOCAL_SIZE if trunc else w
    out = np.zeros((len(rows), w), dtype=np.int64)
    for ly, py in enumerate(rows):
        if py >= 0:
            out[ly, :col_lim] = spp[py, :col_lim]
    return out


def block_groups(n_local):
    """ceil(max n / G) of every stream block, [blocks_y, blocks_x]: n_local is the geometric sample count per pixel over the
    launch's local rows"""
    rows, w = n_local.shape
    g = stream_grid(w, rows)
    padded = np.zeros((g.blocks_y * 8, g.blocks_x * 8), dtype=np.int64)
    padded[:rows, :w] = n_local
    nmax = padded.reshape(g.blocks_y, 8, g.blocks_x, 8).max(axis=(1, 3))
    return (nmax + G - 1) // G


def stream_bytes(n_local, bytes_per_voxel):
    """what VolumeCopies::ensureRayStream allocates for the geometric counts n_local: the samples (whole groups of G for all 64
    lanes of a block, + 16 bytes of slack), a 16-bit count per lane, a 64-bit offset per block and one more"""
    groups = block_groups(n_local)
    blocks = groups.size
    return int(groups.sum()) * 64 * G * bytes_per_voxel + 16 + blocks * 64 * 2 + (blocks + 1) * 8


def look_block(eye, look, view_plane_dist=4.0, up_hint=(0.0, 1.0, 0.0)):
    """the camera block of an eye that looks along `look` (tests/offset_limits.py: corner_camera's layout)"""
    eye = np.asarray(eye, dtype=np.float64)
    look = np.asarray(look, dtype=np.float64)
    look = look / np.linalg.norm(look)
    side = np.cross(look, np.asarray(up_hint, dtype=np.float64)); side /= np.linalg.norm(side)
    up = np.cross(side, look)
    b = np.zeros(21, dtype=np.float32)
    b[0:3] = side; b[4:7] = up; b[8:11] = -look; b[12:15] = eye; b[15] = 1
    b[16:19] = eye; b[19] = 1
    b[20] = view_plane_dist
    return b


def box_half(dims, spacing):
    """half the box's extent along x, y, z in the default view (VolumeRenderer.cs:65-83)"""
    return np.array(dims, dtype=np.float64) / max(dims) * np.array(spacing, dtype=np.float64) / 2.0


def params(oracle, size, cam, alpha, window, mode="grey", lut=None, spacing=(1.0, 1.0, 1.0), view="front", trunc=False,
           row_range=None, threads=4):
    """the oracle's parameters of a frame; lut: the handle's 256-entry table for the modes with a transfer function"""
    assert ("tf" in mode) == (lut is not None), mode
    return oracle.OracleParams(size[0], size[1], cam=cam, alpha_scale=alpha, voxel_size=spacing, min_val=window[0], max_val=window[1],
                               is_mip=int(mode in ("mip", "mip_tf")), view_top=int(view == "top"), view_bottom=int(view == "bottom"),
                               trunc_grid=int(trunc), row_begin=0 if row_range is None else row_range[0],
                               row_end=-1 if row_range is None else row_range[1], tf_rgba=lut, threads=threads)


def geometric_counts(oracle, vol, size, cam, spacing=(1.0, 1.0, 1.0), view="front", window=(0, 255)):
    """n of every ray: with alpha_scale = 0 dest.a stays 0, so the oracle's per-pixel sample count is the count pass's"""
    return oracle.render(vol, params(oracle, size, cam, 0.0, window, spacing=spacing, view=view), want_spp=True)[2]


# ---------------------------------------------------------------------------------------------------------------
# B1: the scan with more than one block per thread
# ---------------------------------------------------------------------------------------------------------------
# size -> (blocks, per, first idle thread, cut-short thread)
SCAN_SIZES = {
    (256, 256): (1024, 1, None, None),          # the boundary: the last size at which every thread has one block
    (328, 264): (1496, 2, 748, None),
    (520, 264): (2312, 3, 771, 770),            # thread 770 has blocks 2310 and 2311 only
    (600, 456): (4408, 5, 882, 881),            # thread 881 has three of five
}
SCAN_ALPHA = 0.05

# ---------------------------------------------------------------------------------------------------------------
# B2: blocks cut by the image edge
# ---------------------------------------------------------------------------------------------------------------
PARTIAL_SIZES = [(101, 77), (97, 65), (8, 8)]
# (the poses of these sizes: PARTIAL_POSES, below RESIDUE_POSES)
PARTIAL_ROW_RANGE = (13, 59)                    # begins and ends inside a block
PARTIAL_STRIPES = (16, 1, 3)                    # rows 16..31 and 64..76 of 77: the second stripe is cut by the image


def cut_blocks(size, trunc=False):
    """(blocks with lanes inside and outside the image, blocks wholly outside it) of a full frame"""
    w, h = size
    rows = local_rows(h, trunc=trunc)
    inside = local_counts(np.ones((h, w), dtype=np.int64), rows, trunc)
    g = stream_grid(w, len(rows))
    padded = np.zeros((g.blocks_y * 8, g.blocks_x * 8), dtype=np.int64)
    padded[:h, :w] = inside
    live = padded.reshape(g.blocks_y, 8, g.blocks_x, 8).sum(axis=(1, 3))
    return int(np.count_nonzero((live > 0) & (live < 64))), int(np.count_nonzero(live == 0))


# ---------------------------------------------------------------------------------------------------------------
# B4: the step cap
# ---------------------------------------------------------------------------------------------------------------
CAP_DIMS = (16384, 4, 4)
CAP_SPACING = (1.0, 512.0, 512.0)               # the box is 1 x 0.125 x 0.125: power-of-two extents
CAP_SIZE = (96, 64)
CAP_ALPHA = 0.0001
CAP_WINDOW = (0, 255)


def cap_volume():
    return np.random.default_rng(16384).integers(0, 256, size=CAP_DIMS[::-1], dtype=np.uint8)


def cap_camera():
    """outside the +x face, looking down the 16384-voxel axis"""
    return look_block((0.6, 0.0, 0.0), (-1.0, 0.0, 0.0), 4.0)


# ---------------------------------------------------------------------------------------------------------------
# B5: where a ray ends inside a group of four
# ---------------------------------------------------------------------------------------------------------------
RESIDUE_DIMS = (64, 64, 64)
RESIDUE_SIZE = (96, 80)
RESIDUE_ALPHAS = (1.0, 0.3, 0.004)
RESIDUE_MIN_RAYS = 20
# The default camera faces the cube: every block's longest ray has 113 samples, 29 groups -- one residue of the BLOCK's group
# count, which is what load_group clamps at.  The second pose looks at an edge: its blocks cover all four.
RESIDUE_POSES = ((), ((0.0, 0.66, -1.65),))           # a pose: the cameraOrient calls after a reset
RESIDUE_MIN_BLOCKS = 10

# B2's poses.  From the default camera the box covers the middle of the image only: no ray of a block at the image's edge has a sample, so
# a cut block holds nothing on either side of the cut.  The third pose dollies in to one unit from the centre, where the box
# fills the image and beyond: the cut blocks' lanes inside the image have samples, and so would their lanes outside it.
CLOSE_POSE = ((1.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 0.3, 0.2))
PARTIAL_POSES = RESIDUE_POSES + (CLOSE_POSE,)


def pose_block(oracle, pose):
    c = oracle.Camera()
    for call in pose:
        c.orient(*call)
    return c.block()


def residue_cameras(oracle):
    return [(pose, pose_block(oracle, pose)) for pose in RESIDUE_POSES]


def residue_volume(oracle, kind):
    return oracle.gen_noise_ball(RESIDUE_DIMS, 1, 0x1234) if kind == "u8" else oracle.gen_noise_ball(RESIDUE_DIMS, 2, 0x5678)


def residue_window(kind):
    return (0, 255) if kind == "u8" else (0, 4095)


def residue_bins(spp, alpha_channel, n_geo):
    """rays per spp % 4 that end by opacity, rays per spp % 4 that end geometrically, rays per ceil(n / G) % DEPTH.  A ray
    ended by opacity when it stopped before its geometric count"""
    hit = n_geo > 0
    early = hit & (spp < n_geo)
    assert not (early & (alpha_channel < END_ALPHA)).any()       # nothing else stops a ray short of n
    geometric = hit & ~early
    groups = (n_geo[hit] + G - 1) // G
    return (np.bincount(spp[early] % G, minlength=G), np.bincount(spp[geometric] % G, minlength=G),
            np.bincount(groups % DEPTH, minlength=DEPTH))


# value, alpha, the sample count at which dest.a has reached 0.95.  s = value / 255 and a = s * alpha per sample;
# dest.a = 1 - (1 - a)^k.  a = 0.25: 0.75^10 = 0.0563, 0.75^11 = 0.0422 -> 11 = 4 * 2 + 3 samples, the fourth of its group is the
# first one left out; a = 0.23: 0.77^11 = 0.0564, 0.77^12 = 0.0434 -> 12 = 4 * 3, a whole group is the first left out.  Both
# are far enough from 0.05 for fp32 not to matter.
CONSTANT_CASES = [(204, 0.3125, 11), (204, 0.2875, 12)]


def constant_volume(value, kind="u8"):
    return np.full(RESIDUE_DIMS[::-1], value, dtype=np.uint8 if kind == "u8" else np.uint16)


# ---------------------------------------------------------------------------------------------------------------
# B6 / B8: the size of the stream
# ---------------------------------------------------------------------------------------------------------------
BYTES_CASES = [((96, 80), None), ((101, 77), None), ((96, 80), (16, 56)), ((101, 77), (13, 59))]     # size, row range
REFUSAL_SIZE = (256, 256)
REFUSAL_DOLLY_STEPS = 2                         # view B: cameraOrient(-1, 0, 0) that many times (a call moves the eye one unit)


def refusal_cameras(oracle):
    """view A: the default camera, 3 units from the centre; view B: the same, dollied out to 5"""
    c = oracle.Camera()
    a = c.block()
    for _ in range(REFUSAL_DOLLY_STEPS):
        c.orient(-1.0, 0.0, 0.0)
    return a, c.block()


# ---------------------------------------------------------------------------------------------------------------
# B7: anisotropic spacing, an eye inside the box
# ---------------------------------------------------------------------------------------------------------------
ANISO_DIMS = (40, 56, 24)
ANISO_SPACING = (1.0, 0.8, 1.7)
ANISO_SIZE = (101, 77)
INSIDE_EYE = (0.1, 0.05, 0.2)


def orbit_blocks(oracle):
    """the orbit poses of tests/test_parity_gpu.py"""
    blocks = [("default", oracle.default_camera_block())]
    c = oracle.Camera()
    c.orient(0, 0.06 * 7, 0.06 * 9)
    blocks.append(("orbit_a", c.block()))
    c.orient(0, -0.06 * 15, 0.06 * 31)
    blocks.append(("orbit_b", c.block()))
    c = oracle.Camera()
    c.orient(0, 0.0, -0.06 * 5)
    blocks.append(("orbit_neg", c.block()))
    c = oracle.Camera()
    c.orient(0, -100.0, 0.3)
    blocks.append(("pole", c.block()))
    return blocks


def inside_camera():
    return look_block(INSIDE_EYE, (-0.3, 0.2, -1.0), 2.0)


def aniso_volume(kind):
    rng = np.random.default_rng(7)
    nx, ny, nz = ANISO_DIMS
    return rng.integers(0, 256 if kind == "u8" else 4096, size=(nz, ny, nx)).astype(np.uint8 if kind == "u8" else np.uint16)
