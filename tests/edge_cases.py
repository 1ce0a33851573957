"""TEST INFRASTRUCTURE ONLY -- the volume sampler's edges, for tests/test_mode_edges_{cpu,gpu}.py.

The isosurface, reslice and shading kernels share one sampler (csrc/vr_sampler.h: address terms, x-pair loads, edge clamps,
trilinear lerps).  This is the shared recipe that takes every kernel to where a sampler goes wrong: volumes with an axis of 1 to 8
voxels, the first and the last voxel of the buffer, cameras inside / grazing / far from the box, images smaller than a tile.

Volume kinds.  `corners`: a background below vmax // 3 with the first and the last voxel of the buffer at vmax (255 / 4095), so a
frame that reads either one shows it.  `constant`: one value everywhere, every gradient 0.  `random`: the whole 0..vmax range.

thin_cases(mode, filt) is the seeded list of frames that the CPU file proves sensitive to the two corner voxels and the GPU file
renders; windows and iso values are in STORED units (the handles run with setQuirks(0)).
"""
from collections import namedtuple

import numpy as np

DIMS_POOL = [(1, 1, 1), (2, 2, 2), (2, 3, 5), (5, 1, 3), (4, 4, 4), (1, 9, 1), (3, 3, 3), (8, 8, 8), (9, 5, 4), (7, 5, 3), (17, 1, 2),
             (50, 1, 50), (128, 4, 4)]                              # x, y, z
SPACINGS = [(1.0, 1.0, 1.0), (1.686, 0.836, 1.578)]
IMAGE_SIZES = [(1, 1), (1, 23), (23, 1), (7, 9), (8, 8), (15, 17), (16, 16), (68, 68)]
VIEWS = ("front", "top", "bottom")
DTYPES = (np.uint8, np.uint16)
REDUCTIONS = ("mip", "minip", "mean")
TF_ISO = [0, 60, 140, 255]
TF_RGBA = [[0.2, 0.9, 0.1, 0.0], [0.9, 0.3, 0.2, 0.4], [1.0, 0.8, 0.6, 0.8], [0.5, 0.5, 1.0, 1.0]]
COEFS = [(0.15, 0.65, 0.2, 16), (1.0, 0.0, 0.0, 16), (0.3, 1.7, 0.6, 1), (0.0, 0.9, 0.35, 128), (0.05, 0.4, 0.9, 2)]     # of test_shading_gpu.py
THIN_SIZE = (68, 68)
THIN_ALPHA = 0.3
CAMERAS_PER_VOLUME = 8          # six random ones, one aimed at the first voxel, one at the last (reslice: eight corner planes)
MODE_SEEDS = {"iso": 20261210, "shade": 20261220, "reslice": 20261230}


def vmax_of(dtype):
    return 255 if np.dtype(dtype) == np.uint8 else 4095


def thin_window(dtype):
    return vmax_of(dtype) // 6, vmax_of(dtype)


def thin_iso(dtype):
    return vmax_of(dtype) // 2


def make_volume(rng, kind, dims, dtype):
    """corners | constant | random; indexed [z, y, x]"""
    nx, ny, nz = dims
    vmax = vmax_of(dtype)
    if kind == "corners":
        vol = rng.integers(0, vmax // 3, size=(nz, ny, nx)).astype(dtype)
        vol.flat[0] = vol.flat[-1] = vmax
    elif kind == "constant":
        vol = np.full((nz, ny, nx), int(rng.integers(1, vmax + 1)), dtype=dtype)
    elif kind == "random":
        vol = rng.integers(0, vmax + 1, size=(nz, ny, nx)).astype(dtype)
    else:
        raise ValueError(kind)
    return vol


def random_camera_block(rng, radius_lo=0.2, radius_hi=4.0):
    """random eye + orthonormal basis looking roughly at the box (also from inside / grazing)"""
    d = rng.normal(size=3); d /= np.linalg.norm(d)
    eye = d * rng.uniform(radius_lo, radius_hi)
    target = rng.uniform(-0.45, 0.45, size=3)
    look = target - eye; look /= np.linalg.norm(look)
    up0 = rng.normal(size=3)
    side = np.cross(look, up0); side /= np.linalg.norm(side)
    up = np.cross(side, look)
    b = np.zeros(21, dtype=np.float32)
    b[0:3] = side; b[4:7] = up; b[8:11] = -look; b[12:15] = eye; b[15] = 1
    b[16:19] = eye; b[19] = 1
    b[20] = rng.uniform(1.0, 5.0)          # view_plane_dist (FOV 22..90 degrees)
    return b


def voxel_centre_in_box(dims, spacing, view, ijk):
    """box coordinates (the camera's) of the centre of voxel (i, j, k): the inverse of cartesianToTextureCoord (VolumeRenderer.cs:175-192)
    under the view's axis swizzle, in float64"""
    swz = view in ("top", "bottom")
    d = np.array([dims[0], dims[2] if swz else dims[1], dims[1] if swz else dims[2]], dtype=np.float64)
    s = np.array([spacing[0], spacing[2] if swz else spacing[1], spacing[1] if swz else spacing[2]], dtype=np.float64)
    ext = d / max(dims) * s
    tc = (np.array(ijk, dtype=np.float64) + 0.5) / np.array(dims, dtype=np.float64)
    if view == "top":
        u = np.array([tc[0], tc[2], tc[1]])
    elif view == "bottom":
        u = np.array([tc[0], 1.0 - tc[2], 1.0 - tc[1]])
    else:
        u = np.array([tc[0], tc[1], 1.0 - tc[2]])
    return u * ext - ext / 2.0


def aimed_camera_block(rng, target, dist_lo=0.05, dist_hi=0.6):
    """an eye at a random direction and distance from `target` (box coordinates) that looks straight at it, FOV 22..37 degrees"""
    d = rng.normal(size=3); d /= np.linalg.norm(d)
    eye = target + d * rng.uniform(dist_lo, dist_hi)
    look = -d
    side = np.cross(look, rng.normal(size=3)); side /= np.linalg.norm(side)
    up = np.cross(side, look)
    b = np.zeros(21, dtype=np.float32)
    b[0:3] = side; b[4:7] = up; b[8:11] = -look; b[12:15] = eye; b[15] = 1
    b[16:19] = eye; b[19] = 1
    b[20] = rng.uniform(3.0, 5.0)
    return b


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def differ(got, want):
    """'' when the tuples agree (float32 arrays by bits, integer arrays by value), else what differs"""
    out = []
    for k, (g, w) in enumerate(zip(got, want)):
        if g.shape != w.shape:
            out.append(f"array {k}: shape {g.shape} vs {w.shape}")
            continue
        bad = (bits(g) != bits(w)) if g.dtype == np.float32 else (g != w)
        if bad.any():
            at = tuple(int(i) for i in np.argwhere(bad)[0])
            out.append(f"array {k}: {int(bad.sum())} entries differ, first at {at}: {g[at]} vs {w[at]}")
    return "; ".join(out)


def depends_on_voxel(render_ref, vol, flat_index):
    """render_ref(volume) -> a tuple of arrays.  The reference's frame with that voxel at vmax and with it at 0: True when any
    output differs in its bits, i.e. when the frame reads the voxel (a kernel that read it as 0 would be seen)"""
    frames = []
    for value in (vmax_of(vol.dtype), 0):
        v = vol.copy()
        v.flat[flat_index] = value
        frames.append(render_ref(v))
    return bool(differ(frames[0], frames[1]))


# ---------------------------------------------------------------------------------------------------------------
# the seeded thin-volume frames
# ---------------------------------------------------------------------------------------------------------------
# cam: the camera block (iso, shade); geom / n / red: the plane, the slab length and the reduction (reslice)
Case = namedtuple("Case", "what dims dtype spacing view layout skip tf coef cam geom n red")
Group = namedtuple("Group", "dims dtype vol cases")           # one resident volume, its frames


def corner_plane(rng, dims, size, n, step=None):
    """An oblique plane that holds the first and the last voxel of the volume: one pixel in the lower left quarter of the image
    lands within 0.3 voxels of voxel (0, 0, 0)'s centre, one in the upper right quarter within 0.3 voxels of the last voxel's, so
    the image spans the box along its diagonal with a margin outside it; across the diagonal the pixel pitch is drawn freely and
    the plane is turned about the diagonal at random.  Slab steps run along the plane's normal, `step` or 0.2 to 1.5 voxels long."""
    w, h = size
    first = rng.uniform(-0.3, 0.3, size=3)
    last = np.array(dims, dtype=np.float64) - 1.0 + rng.uniform(-0.3, 0.3, size=3)
    p0 = np.array([rng.integers(w // 8, w // 3 + 1), rng.integers(h // 8, h // 3 + 1)], dtype=np.float64)
    p1 = np.array([rng.integers(w - 1 - w // 3, w - w // 8), rng.integers(h - 1 - h // 3, h - h // 8)], dtype=np.float64)
    diag = last - first
    e1 = diag / np.linalg.norm(diag)
    e2 = np.cross(e1, rng.normal(size=3)); e2 /= np.linalg.norm(e2)
    e3 = np.cross(e1, e2)
    a = (p1 - p0) / np.linalg.norm(p1 - p0)
    b = np.array([-a[1], a[0]])
    along = np.linalg.norm(diag) / np.linalg.norm(p1 - p0)            # voxels per pixel along the diagonal
    across = rng.uniform(0.03, 0.3) * (1.0 + sorted(dims)[1]) / 8.0   # ... and across it
    du = along * a[0] * e1 + across * b[0] * e2
    dv = along * a[1] * e1 + across * b[1] * e2
    o = first - p0[0] * du - p0[1] * dv
    dw = (rng.uniform(0.2, 1.5) if step is None else step) * e3
    return np.concatenate([o, du, dv, dw]).astype(np.float32)


def pick(rng, options):
    """one of `options`, drawn: settings drawn per frame share no period with the loops around them, as cycled ones would"""
    return options[int(rng.integers(len(options)))]


def thin_cases(mode, filt):
    """mode: iso | shade | reslice.  Per pool entry and voxel type one `corners` volume and CAMERAS_PER_VOLUME frames of it at
    68 x 68 (random_camera_block: eyes inside the box, grazing it and far from it).  Layout, skipping, view, spacing, transfer
    function, shading coefficients and reduction are drawn per frame from a generator of their own, not multiplied out; the slab
    length runs through 1..9 (a period that shares nothing with the 8 frames of a volume)."""
    rng = np.random.default_rng(MODE_SEEDS[mode] + filt)
    opt = np.random.default_rng(MODE_SEEDS[mode] + 5 + filt)
    groups, k = [], 0
    for dims in DIMS_POOL:
        for dtype in DTYPES:
            vol = make_volume(rng, "corners", dims, dtype)
            cases = []
            for c in range(CAMERAS_PER_VOLUME):
                layout, skip, tf = pick(opt, (0, 1)), pick(opt, (0, 1)), pick(opt, (0, 1))
                spacing, view, coef = pick(opt, SPACINGS), pick(opt, VIEWS), pick(opt, COEFS)
                n, red = 1 + k % 9, pick(opt, REDUCTIONS)
                cam = geom = None
                if mode == "reslice":
                    geom = corner_plane(rng, dims, THIN_SIZE, n)
                    what = f"{mode} filt {filt} {dims} {np.dtype(dtype).name} frame {c}: layout {layout} tf {tf} {red} n {n}"
                else:
                    if c < 6:
                        cam = random_camera_block(rng)
                    else:         # a corner voxel of a long volume is a small part of a frame that shows the whole box: look at it
                        ijk = (0, 0, 0) if c == 6 else tuple(v - 1 for v in dims)
                        cam = aimed_camera_block(rng, voxel_centre_in_box(dims, spacing, view, ijk))
                    what = (f"{mode} filt {filt} {dims} {np.dtype(dtype).name} frame {c}: spacing {spacing} {view} layout {layout} skip {skip} tf {tf}"
                            + (f" coef {coef}" if mode == "shade" else ""))
                cases.append(Case(what, dims, dtype, spacing, view, layout, skip, tf, coef, cam, geom, n, red))
                k += 1
            groups.append(Group(dims, dtype, vol, cases))
    return groups


def thin_params(oracle, case, filt, lut):
    """the oracle.OracleParams of an iso / shade frame of thin_cases (lut: the transfer function's 256 entries)"""
    lo, hi = thin_window(case.dtype)
    return oracle.OracleParams(THIN_SIZE[0], THIN_SIZE[1], cam=case.cam, alpha_scale=THIN_ALPHA, voxel_size=case.spacing, min_val=lo, max_val=hi,
                               view_top=int(case.view == "top"), view_bottom=int(case.view == "bottom"), filter=filt,
                               tf_rgba=lut if case.tf else None)


def thin_reference(refs, oracle, mode, case, filt, lut, vol):
    """the CPU definition's frame of a thin_cases frame on `vol`: every output array of the mode.
    refs: {"iso" | "shade" | "reslice": (the binding module, its built library)}"""
    binding, lib = refs[mode]
    if mode == "reslice":
        lo, hi = thin_window(case.dtype)
        return binding.render(lib, vol, case.geom, THIN_SIZE[0], THIN_SIZE[1], mode=case.red, n=case.n, filt=filt, min_val=lo, max_val=hi,
                              tf_rgba=lut if case.tf else None, u16_offset=False)
    p = thin_params(oracle, case, filt, lut)
    if mode == "iso":
        return binding.render(lib, vol, p, thin_iso(case.dtype), u16_offset=False)
    return binding.render(lib, vol, p, *case.coef)
