"""TEST INFRASTRUCTURE ONLY -- the 16-bit range scan's skipped voxel and what the exact range selects, for
tests/test_range_scan_cpu.py and tests/test_range_scan_gpu.py.

Every 16-bit load runs one scan (stats_kernel pass 0, csrc/vr_helpers.hip) that yields two ranges.  The REFERENCE's range
(src/RendererCore.cpp:361-379) leaves out the voxel at linear index 8390640 -- X below -- and sets the dataset range, the
default window and the histogram's scale.  The EXACT range includes X and selects everything that trusts the voxels' values: the
12-bit packed volume copy and its base, the 12-bit ray-stream format and its base, the instances that index the window table
without clamping, the skip-order signature.  The two differ only when an extreme value sits at X; the volumes here are the
smallest that have a voxel there.

Volumes are indexed [z, y, x]; dims are (nx, ny, nz); sizes are (width, height); windows are in STORED units (the handles run
with setQuirks(0)).
"""
import functools
import importlib.util
from collections import namedtuple
from pathlib import Path

import numpy as np

_spec = importlib.util.spec_from_file_location("edge_cases", Path(__file__).resolve().parent / "edge_cases.py")
E = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(E)

SKIPPED_INDEX = 8390640             # `if(i == 8390640) continue;`
BRICK = 4                           # 4 x 4 x 4 voxels per brick (csrc/vr_frame.h)

# no_x: X does not exist (the volume has exactly 8390640 voxels), nothing is skipped.  x_last: X is the last voxel.  x_plane: X
# = (240, 7, 128), in the only plane of a partial last brick layer and of a partial last layer of skip-grid cells
SHAPES = {"no_x": (34961, 16, 15), "x_last": (4091, 293, 7), "x_plane": (256, 256, 129)}
WITH_X = ("x_last", "x_plane")
KINDS = ("low_in_span", "high_in_span", "high_out", "low_out")
IN_SPAN = ("low_in_span", "high_in_span")

# kind -> (the background's minimum, its span, X's value).  The background reaches both of its ends (two pinned voxels), so
# the reference's range of a volume with X is (base, base + span) and the exact range is that with X's value at one end
Kind = namedtuple("Kind", "base span x")
KIND = {
    "low_in_span": Kind(1100, 3900, 1000),       # exact span 4000: packs; a base taken from the reference's minimum wraps X
    "high_in_span": Kind(1100, 3000, 4190),      # exact span 3090: packs; the default window ends 90 below X
    "high_out": Kind(1100, 3000, 60000),         # reference span 3000, exact span 58900: nothing may pack
    "low_out": Kind(30000, 3000, 0),             # the mirror: exact span 33000
}
U8_BACKGROUND_MAX, U8_X, U8_WINDOW = 200, 255, (0, 200)


def linear_index(dims, ijk):
    return ijk[0] + dims[0] * (ijk[1] + dims[1] * ijk[2])


def coords_of(dims, lin):
    """(i, j, k) of a linear index, or None when the volume ends before it"""
    nx, ny, nz = dims
    if lin >= nx * ny * nz:
        return None
    return lin % nx, (lin // nx) % ny, lin // (nx * ny)


def bricked_index(dims, ijk):
    """storage_index(layout 1, ...) of csrc/vr_helpers.hip: bricks x fastest, 64 voxels each, x fastest inside"""
    bnx, bny = (dims[0] + BRICK - 1) // BRICK, (dims[1] + BRICK - 1) // BRICK
    i, j, k = ijk
    brick = i // BRICK + bnx * (j // BRICK + bny * (k // BRICK))
    return brick * 64 + (i % BRICK) + BRICK * (j % BRICK) + BRICK * BRICK * (k % BRICK)


def x_of(shape):
    return coords_of(SHAPES[shape], SKIPPED_INDEX)


# ---------------------------------------------------------------------------------------------------------------
# the reference's arithmetic
# ---------------------------------------------------------------------------------------------------------------
def reference_range(vol):
    """src/RendererCore.cpp:361-379: 8-bit volumes get (0, 255); 16-bit ones the minimum and maximum over the linear order
    i + nx * (j + ny * k) without index SKIPPED_INDEX, from the initial values 9000000 and -1"""
    if vol.dtype == np.uint8:
        return 0, 255
    flat = vol.reshape(-1)
    if flat.size > SKIPPED_INDEX:
        flat = np.concatenate([flat[:SKIPPED_INDEX], flat[SKIPPED_INDEX + 1:]])
    if flat.size == 0:
        return 9000000, -1
    return int(flat.min()), int(flat.max())


def reference_histogram(vol):
    """src/RendererCore.cpp:386-405 operation by operation in float32 -- the arithmetic of reference_histogram in
    tests/test_u16_full_range_gpu.py with the scale and the normaliser's start taken from reference_range (every voxel is
    counted, X too: only the range loop skips).  Returns (bins, whether the largest count raised the normaliser)"""
    f32 = np.float32
    if vol.dtype == np.uint8:
        b, vmax = vol.reshape(-1).astype(np.int64), -1
    else:
        vmax = reference_range(vol)[1]
        x = (vol.astype(f32).ravel() * f32(255.0)).astype(f32) / f32(vmax)
        b = np.floor(x.astype(np.float64) + 0.5).astype(np.int64) & 0xFFFF      # std::round of a value >= 0; stored to uint16_t
    counts = np.bincount(b[(b != 0) & (b < 256)], minlength=256)
    norm = max(vmax, int(counts.max()))
    return (counts.astype(f32) * f32(100.0) / f32(norm)).astype(f32), norm > vmax


# ---------------------------------------------------------------------------------------------------------------
# the volume family
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def unit_field(shape):
    """the smooth field of u16_volumes.smooth12 in [0, 1] (float32), by broadcasting: 8.4 M voxels"""
    nx, ny, nz = SHAPES[shape]
    x, y, z = np.arange(nx, dtype=np.float32), np.arange(ny, dtype=np.float32), np.arange(nz, dtype=np.float32)
    f = np.sin(x * np.float32(0.3))[None, None, :] + np.cos(y * np.float32(0.23))[None, :, None] + np.sin(z * np.float32(0.31))[:, None, None]
    return ((f + np.float32(3.0)) / np.float32(6.0)).astype(np.float32)


def background(shape, span, dtype=np.uint16):
    """smooth data with a little noise on top in [0, span]; voxels 0 and 1 of the buffer pinned to 0 and span"""
    rng = np.random.default_rng(span + SHAPES[shape][0])
    v = (unit_field(shape) * np.float32(span)).astype(np.int32)
    v += rng.integers(0, 3, size=v.shape, dtype=np.int32)
    v = np.clip(v, 0, span).astype(dtype)
    v.flat[0], v.flat[1] = 0, span
    return v


@functools.lru_cache(maxsize=6)
def volume(shape, kind, at=SKIPPED_INDEX):
    """kind's background with kind's extreme value at linear index `at` (SKIPPED_INDEX - 1: the twin whose two ranges are
    equal); a volume that ends before `at` is the background alone.  Read-only: shared between tests"""
    base, span, x = KIND[kind]
    v = background(shape, span)
    v += np.uint16(base)
    if at < v.size:
        v.flat[at] = x
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=2)
def volume_u8(shape):
    """an 8-bit volume whose only 255 is X"""
    v = background(shape, U8_BACKGROUND_MAX, np.uint8)
    v.flat[SKIPPED_INDEX] = U8_X
    v.setflags(write=False)
    return v


def exact_range(vol):
    return int(vol.min()), int(vol.max())


def flat_with_peak(shape, floor=1000, peak=3000):
    """a flat background with one bright voxel at X (for smoothVolume)"""
    nx, ny, nz = SHAPES[shape]
    v = np.full((nz, ny, nx), floor, dtype=np.uint16)
    v.flat[SKIPPED_INDEX] = peak
    return v


def zeros_but_x(shape, x_value):
    nx, ny, nz = SHAPES[shape]
    v = np.zeros((nz, ny, nx), dtype=np.uint16)
    v.flat[SKIPPED_INDEX] = x_value
    return v


# ---------------------------------------------------------------------------------------------------------------
# cameras zoomed on X, and the proof that a frame reads it
# ---------------------------------------------------------------------------------------------------------------
# out: from X towards the eye in box coordinates (X lies on the box's -z face in both shapes; x_last's X is its +x +y corner
# too); dist: eye to X's centre; vpd: view_plane_dist.  At X a frame is 2 * dist * (w / h) / vpd wide: a few tens of voxels.
# The facing and oblique views enter the box at X (the first sample of a ray); the through views look from the far side at a
# low opacity, so X is the LAST sample of rays that cross the whole volume.
View = namedtuple("View", "name shape size out dist vpd alpha")
VIEWS = [
    View("plane_facing", "x_plane", (48, 32), (0.0, 0.0, -1.0), 0.12, 4.0, 0.3),
    View("plane_oblique", "x_plane", (37, 29), (-0.55, 0.45, -0.7), 0.2, 6.0, 0.3),
    View("plane_through", "x_plane", (33, 32), (0.05, 0.08, 1.0), 0.65, 20.0, 0.01),
    View("last_facing", "x_last", (48, 32), (0.02, 0.03, -1.0), 0.008, 4.0, 0.3),
    View("last_oblique", "x_last", (37, 29), (0.5, 0.35, -0.8), 0.012, 5.0, 0.3),
    View("last_through", "x_last", (33, 32), (-0.3, -0.2, 1.0), 0.01, 5.0, 0.05),
]
VIEWS_OF = {s: [v for v in VIEWS if v.shape == s] for s in WITH_X}
BAND = 7                            # the proof renders the rows within BAND of the image's middle, where the camera looks


def camera_block(view):
    """an eye at `dist` from X's centre along `out` that looks straight at it (the block of tests/offset_limits.corner_camera)"""
    dims = SHAPES[view.shape]
    target = E.voxel_centre_in_box(dims, (1.0, 1.0, 1.0), "front", x_of(view.shape))
    out = np.array(view.out, dtype=np.float64)
    out /= np.linalg.norm(out)
    eye = target + view.dist * out
    look = -out
    side = np.cross(look, np.array([0.0, 1.0, 0.0])); side /= np.linalg.norm(side)
    up = np.cross(side, look)
    b = np.zeros(21, dtype=np.float32)
    b[0:3] = side; b[4:7] = up; b[8:11] = -look; b[12:15] = eye; b[15] = 1
    b[16:19] = eye; b[19] = 1
    b[20] = view.vpd
    return b


def params(oracle, view, window, mode="grey", lut=None, rows=None):
    w, h = view.size
    return oracle.OracleParams(w, h, cam=camera_block(view), alpha_scale=view.alpha, min_val=window[0], max_val=window[1],
                               is_mip=int(mode == "mip"), tf_rgba=lut if mode == "tf" else None,
                               row_begin=0 if rows is None else rows[0], row_end=-1 if rows is None else rows[1])


def band(view):
    h = view.size[1]
    return max(h // 2 - BAND, 0), min(h // 2 + BAND, h)


def affected_pixels(oracle, vol, view, window):
    """The pixels (y, x) of the grey composite frame of `vol` under `window` that read X: oracle.render of the volume against
    oracle.render of the same volume with X at the OTHER end of the window (X itself classifies as the end it lies at or beyond),
    on the rows of band(view).  Empty: the frame does not sample X and tests nothing about it"""
    flat = vol.reshape(-1)
    x = int(flat[SKIPPED_INDEX])
    other = window[0] if x >= window[1] else window[1]
    assert x <= window[0] or x >= window[1], (x, window)
    rows = band(view)
    p = params(oracle, view, window, rows=rows)
    a = oracle.render(vol, p)[0]
    moved = vol.copy()
    moved.reshape(-1)[SKIPPED_INDEX] = other
    b = oracle.render(moved, p)[0]
    bad = (a.view(np.uint32) != b.view(np.uint32)).any(axis=2)
    assert not bad[:rows[0]].any() and not bad[rows[1]:].any()
    return np.argwhere(bad)


def skip_window(kind):
    """a window whose lower end lies above the whole background and at or below X: every cell but X's neighbourhood is skipped"""
    assert kind == "high_out"
    k = KIND[kind]
    return k.base + k.span + 900, k.x


def default_window(kind):
    """the reference's range of kind's volumes: the window of a fresh load.  X lies outside it"""
    k = KIND[kind]
    return k.base, k.base + k.span


def exact_window(kind):
    """the exact range as a window: every voxel inside it, X at one end (the instances without a clamp)"""
    k = KIND[kind]
    return min(k.base, k.x), max(k.base + k.span, k.x)


def render_cases():
    """every (view, kind or "u8", window) the GPU file renders: the default and the exact window of each kind, the skipping
    window for high_out, (0, 200) for the 8-bit twin"""
    out = []
    for view in VIEWS:
        for kind in KINDS:
            out.append((view, kind, default_window(kind)))
            out.append((view, kind, exact_window(kind)))
        out.append((view, "high_out", skip_window("high_out")))
        out.append((view, "u8", U8_WINDOW))
    return out


def case_volume(shape, kind):
    return volume_u8(shape) if kind == "u8" else volume(shape, kind)
