/*
 * vr_core.h -- C ABI of libvr_core.so, the MI355X (gfx950) replacement for the GPU
 * ray-march path of gallickgunner/Volume-Renderer.
 *
 * The reference has no FFI: the boundary is the C++ surface of `RendererCore`
 * (include/RendererCore.h:9-44) as used by its only caller `RendererGUI`
 * (a friend class, src/RendererGUI.cpp).  Each entry point below names the
 * reference member / call site it replaces.  All calls are single-threaded per
 * handle, like the reference (everything runs on the GL thread).
 *
 * Conventions: functions returning `int` return 0 (VR_OK) on success and a
 * VR_E_* code otherwise; the text is available from vr_last_error().
 * Recoverable errors that the reference reports through its `title`/`msg`
 * strings (src/RendererGUI.cpp:90-95) are ALSO queued for vr_take_message().
 * Nothing here falls back to a CPU renderer: without a HIP device vr_render()
 * fails with VR_E_NO_DEVICE.
 */
#ifndef VR_CORE_H
#define VR_CORE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vr_renderer *vr_handle;

enum {
    VR_OK = 0,
    VR_E_INVALID = 1,     /* bad argument / call order                        */
    VR_E_NO_DEVICE = 2,   /* no HIP device (or host-only handle) for a GPU op */
    VR_E_HIP = 3,         /* HIP runtime error                                */
    VR_E_IO = 4,          /* file open / parse error                          */
    VR_E_NOMEM = 5
};

/* NEAREST: what the reference's texture() yields -- its GL_LINEAR on an integer texture is refused by a conformant GL (all-zero
   frame) and read as NEAREST by the drivers it was written on; frames are bit-identical to the reference shader executed under
   Mesa llvmpipe (tests/golden/ref_gl/).  TRILINEAR (north-star's filter; no reference semantics): GL's linear rule with
   CLAMP_TO_EDGE, x then y then z, each lerp one fma -- bit-identical to llvmpipe's GL_LINEAR on an R32F texture of the same
   voxels through the reference shader with `usampler3D` spelled `sampler3D` (tests/golden/ref_gl/tri_*). */
enum { VR_FILTER_NEAREST = 0, VR_FILTER_TRILINEAR = 1 };
enum { VR_ACCUM_ITERATIVE = 0, VR_ACCUM_CLOSED_FORM = 1 };
enum { VR_LAYOUT_LINEAR = 0, VR_LAYOUT_BRICKED = 1 };
enum { VR_SYNTH_SPHERE_U8 = 0, VR_SYNTH_NOISE_BALL = 1,
       VR_SYNTH_NOISE_BALL_CT = 2 /* 16-bit only: the noise ball + 1000, i.e. stored the way the reference expects CT data (src/RendererCore.cpp:66-67) */ };

/* quirk switches (SURVEY.md section 8(a) quirk list); default = VR_QUIRK_DEFAULT */
enum {
    VR_QUIRK_TRUNC_GRID = 1u << 0,   /* Q1: dispatch W/16 x H/16 groups, drop the rest
                                        (src/RendererCore.cpp:121-122). Default OFF. */
    VR_QUIRK_U16_OFFSET = 1u << 1,   /* Q10: +1000 on min/max for 16-bit data
                                        (src/RendererCore.cpp:66-67,77-78). Default ON. */
    VR_QUIRK_DEFAULT = VR_QUIRK_U16_OFFSET
};

/* ---- lifetime: RendererCore::RendererCore / ~RendererCore / setup()
        (src/RendererCore.cpp:13-44; RendererGUI.cpp:38-40) ------------------- */
/* device >= 0: HIP device ordinal.  device = -1: host-only handle (camera, file
   parsing, transfer-function building work; every GPU operation fails loudly). */
int vr_create(vr_handle *out, int device);
void vr_destroy(vr_handle h);
/* window_size / framebuffer_size + setup(): allocates the RGBA32F off-screen
   target fb_w x fb_h in HBM (setupFBO, src/RendererCore.cpp:184-219). */
int vr_setup(vr_handle h, int win_w, int win_h, int fb_w, int fb_h);
const char *vr_last_error(vr_handle h);
/* msg/title polling (src/RendererGUI.cpp:90-95): returns 1 and fills the buffers
   if a message was pending (and clears it), 0 otherwise. */
int vr_take_message(vr_handle h, char *title, size_t title_cap, char *msg, size_t msg_cap);

/* ---- camera: Camera::setOrientation / resetCamera / setUBO
        (src/Camera.cpp:30-151; bound at RendererGUI.cpp:42-46, :363) ---------- */
int vr_camera_orient(vr_handle h, float zoom, float zenith, float azimuth);
int vr_camera_reset(vr_handle h);
/* Camera::setViewMatrix(eye, side, up, look_at) (include/Camera.h:18, src/Camera.cpp:46-57):
   four xyzw vectors; the members are normalised, the matrix is built from the arguments as
   given (columns side, up, -look_at, eye), exactly like the reference */
int vr_camera_set_view_matrix(vr_handle h, const float eye4[4], const float side4[4], const float up4[4],
                              const float look_at4[4]);
int vr_camera_set_block(vr_handle h, const float block21[21]);
int vr_camera_get_block(vr_handle h, float block21[21]);

/* ---- shader: loadShader(fn, reload) (src/RendererCore.cpp:112-136;
        RendererGUI.cpp:51,144,216).  The HIP kernel is built in; this records the
        name (so `loaded_shader` is non-empty) and computes workgroups_x/y. ------ */
int vr_load_shader(vr_handle h, const char *path, int reload);
int vr_workgroups(vr_handle h, int *wg_x, int *wg_y);
const char *vr_loaded_shader(vr_handle h);
const char *vr_loaded_dataset(vr_handle h);

/* ---- volume: readVolumeData / checkRawInfFile (src/RendererCore.cpp:46-54,
        242-447; RendererGUI.cpp:196-197,209) --------------------------------- */
int vr_check_raw_inf_file(vr_handle h, const char *path);          /* 1 = sidecar exists */
/* tex3D_dim / voxel_size as typed into the raw-inf panel (RendererGUI.cpp:423-429):
   used when a .raw has no .inf sidecar (the sidecar is then written). */
int vr_set_dims(vr_handle h, int nx, int ny, int nz);
int vr_set_spacing(vr_handle h, float sx, float sy, float sz);
/* datasize_bytes = 1|2 (RendererGUI.cpp:128,134).  64-bit sizes throughout (F5). */
int vr_read_volume_file(vr_handle h, const char *path, int datasize_bytes);
/* memory-based loaders (new; the reference only loads files): host pointer is
   copied, x fastest then y then z, host byte order. */
int vr_set_volume(vr_handle h, const void *host_voxels, int nx, int ny, int nz,
                  int datasize_bytes, float sx, float sy, float sz);
/* generate a synthetic volume directly in HBM (never crosses PCIe).
   kind = VR_SYNTH_SPHERE_U8 (param = radius in voxels), VR_SYNTH_NOISE_BALL or VR_SYNTH_NOISE_BALL_CT
   (param = seed). */
int vr_generate_synthetic(vr_handle h, int kind, int nx, int ny, int nz, int datasize_bytes,
                          uint32_t param);
/* copy the resident volume back to the host in x-fastest linear order */
int vr_read_volume(vr_handle h, void *host_voxels, size_t bytes);
int vr_get_dims(vr_handle h, int dims3[3], float spacing3[3], int *datasize_bytes);
/* min_dataset_val / max_dataset_val (src/RendererCore.cpp:360-384) */
int vr_get_dataset_range(vr_handle h, int *min_val, int *max_val);
/* 256-bin display histogram (src/RendererCore.cpp:386-405) */
int vr_histogram(vr_handle h, float hist256[256]);
/* measurement aid (SURVEY 8d "confirm the HBM peak on the box"): best-of-reps streaming read of
   the resident volume with 16-byte loads; *gbps = 1e9 bytes per second.  No reference
   counterpart (the reference reads GL_TIME_ELAPSED only, src/RendererCore.cpp:149-153). */
int vr_measure_stream_read(vr_handle h, int reps, double *gbps);
/* Multi-GPU, one process per GPU: on the rank that received the shards, turn the rank-major gather buffer
   -- n shards of local_rows x fb_w pixels, `channels` floats each (4: RGBA32F, 2: (grey, alpha), see
   vr_set_framebuffer_format) -- into the fb_w x fb_h RGBA32F frame the GUI blits (src/RendererGUI.cpp:158-162):
   one kernel on `hip_stream` (0 = the handle's stream) that undoes the row interleave (stripe_rows > 0: cyclic stripes
   as in vr_set_row_stripes; 0: contiguous blocks as in vr_set_row_range) and expands (grey, alpha).  Both pointers are
   device memory of this handle's device.  vr_group_render() does the same internally. */
int vr_assemble_shards(vr_handle h, const void *gathered_device, void *frame_device, int n, int local_rows, int stripe_rows,
                       int channels, void *hip_stream);

/* ---- PVM / DDS codec (host only, no handle): readPVMvolume of the reference's
        include/ddsbase.h:29-35 (src/ddsbase.cpp:768-858).  Returns a malloc'ed payload of
        width*height*depth*components bytes (free with vr_free) or NULL; 16-bit payloads
        are big-endian as stored (V^3 convention). ---------------------- */
unsigned char *vr_read_pvm_volume(const char *filename, unsigned int *width, unsigned int *height,
                                  unsigned int *depth, unsigned int *components, float *scalex,
                                  float *scaley, float *scalez);
/* the reference's checksum() (src/ddsbase.cpp:869-893) */
unsigned int vr_checksum(const unsigned char *data, unsigned int bytes);
void vr_free(void *p);

/* ---- uniforms: setAlpha / setMIP / setInitialCameraRotation / setMinVal /
        setMaxVal (src/RendererCore.cpp:56-98; RendererGUI.cpp:336-358,382-385) -- */
int vr_set_alpha(vr_handle h, float alpha_scale);
int vr_set_mip(vr_handle h, int use_mip);
int vr_set_view(vr_handle h, int rotate_to_top, int rotate_to_bottom); /* also resets camera */
int vr_set_window(vr_handle h, int min_val, int max_val);
int vr_get_window(vr_handle h, int *min_val, int *max_val);

/* ---- build-defined switches (no reference equivalent) ---------------------- */
int vr_set_filter(vr_handle h, int filter);          /* VR_FILTER_*  (F4)            */
int vr_set_accum(vr_handle h, int accum);            /* VR_ACCUM_*   (Q8)            */
int vr_set_quirks(vr_handle h, uint32_t quirks);     /* VR_QUIRK_*                   */
int vr_set_layout(vr_handle h, int layout);          /* VR_LAYOUT_* (default BRICKED); re-lays the volume out */
int vr_set_skip_empty(vr_handle h, int enable);      /* exact empty-space skipping (north-star's "adaptive step"): frames and sample
                                                        counts are bit-identical with it; NEAREST kernels per ray and batch, the
                                                        LDS-staged TRILINEAR kernel per tile and brick layer (round 5), tiles on
                                                        global taps per ray and batch.  No reference equivalent                  */
/* First-hit isosurface mode (no reference equivalent; the reference's GUI labels CT values in Hounsfield units,
   src/RendererGUI.cpp:371-411).  enable = 1: every frame shows the surface where the sampled data first reach iso_value,
   lit by a headlight, and stores its depth (vr_read_depth); the MIP / composite settings are ignored while it is on and
   kept, so enable = 0 restores the earlier mode unchanged.  Default off.  iso_value is in the units of vr_set_window.
   Per pixel, each step one correctly rounded fp32 operation in the order given (no rsqrt / pow / fast math; the only fused
   operations are TRILINEAR's lerps, as in the composite mode):
   1. Ray and positions: those of the composite mode -- the ray, the box intersection, p0 = start + dir * EPSILON, the
      composite step, both VR_ACCUM_* modes, the view's texture-coordinate mapping, the box-exit test without its dest.a
      term, max_steps.  s_i = the filtered raw voxel value at sample i (before the window), either filter.
   2. Hit: the first step i with s_i >= iso_s; iso_s = float(iso_value + 1000) for 16-bit data under VR_QUIRK_U16_OFFSET,
      float(iso_value) otherwise.
   3. Refinement: i = 0: h = q_0.  Else f = (iso_s - s_{i-1}) / (s_i - s_{i-1}) and per component h = q_{i-1} + f * (q_i - q_{i-1})
      (the difference, then the product, then the sum).
   4. Normal: central differences of the same sampler at h, g_a = S(+1) - S(-1) along each volume axis a -- TRILINEAR at the
      continuous voxel coordinates u +- 1 (u = tc * dim - 0.5), NEAREST at voxel indices i +- 1; clamped to the edge.  Box
      space: G_a = g_b * (dim_b / ext_a) with b the volume axis behind box axis a (front: x, y, z with z negated; top: x, z, y;
      bottom: x, z, y with the last two negated).  N = v * (1 / sqrt(dot)), v = -G, dot = (v_z*v_z + v_y*v_y) + v_x*v_x;
      dot = 0: N = -dir.
   5. Shading, two-sided headlight L = V = H = -dir: d = (N_z*L_z + N_y*L_y) + N_x*L_x, negated when below 0; spec = d^16 by
      four squarings; rgb = min(base * (0.15 + 0.65 * d) + 0.2 * spec, 1), alpha 1.  base = the transfer function's rgb at the
      windowed iso_s (the composite mode's index rule) when one is set, else white.
   6. Miss (the ray leaves the box or runs out of steps): (0, 0, 0, 0), the reference's background.
   7. Depth: t = ((h_z - o_z) * d_z + (h_y - o_y) * d_y) + (h_x - o_x) * d_x; +inf on a miss.
   8. vr_count_samples: the march samples up to and including the hit step (refinement and gradient taps not counted) --
      without a hit the count of a composite frame at alpha_scale 0.
   vr_set_skip_empty applies: a cell whose dilated maximum is below iso_s is not sampled (frames, depth and counts are the
   same bits).  Frames into a VR_FB_GREYALPHA32F target are refused (VR_E_INVALID); a vr_group gathers RGBA, not depth. */
int vr_set_isosurface(vr_handle h, int enable, int32_t iso_value);
/* the last isosurface frame's depth: one float per pixel of the colour target, indexed like it (fb_w x fb_h, or
   vr_local_rows() x fb_w for a compact external target); pixels that frame did not render keep earlier values (+inf
   initially).  VR_E_INVALID before the first isosurface frame. */
int vr_read_depth(vr_handle h, float *depth, size_t n_floats);
/* Multi-planar reslice mode (no reference equivalent): axial, coronal, sagittal or oblique reformats, plain (n = 1) or as a
   thick slab reduced to its maximum (MIP), minimum (MinIP) or mean, and the value behind each pixel (vr_read_reslice_values).
   enable = 1: every frame shows the plane; alpha_scale, the MIP switch, the camera, the view and the spacing are ignored while
   it is on and kept, so enable = 0 restores the earlier mode unchanged.  Default off.  Per pixel, each step one correctly
   rounded fp32 operation in the order given (nothing contracted; the only fused operations are TRILINEAR's lerps, exactly as
   in the isosurface mode):
   1. Geometry: geom12 = o[3], du[3], dv[3], dw[3] in voxel index coordinates (x the fastest volume axis; voxel (i, j, k)'s
      centre at (i, j, k)); o is the centre of pixel (0, 0).  Pixel (x, y) is numbered by the global column and row of the
      colour target (as a full-frame vr_read_pixels); X = (float)x, Y = (float)y, p_a = (o_a + X*du_a) + Y*dv_a.
   2. Slab: n samples, 1 <= n <= 1024; for k = 0 .. n-1, c_k = (float)(2k - (n-1)) * 0.5f (exact), q_a = p_a + c_k*dw_a.
   3. Inside test: r_a = q_a + 0.5f; the sample is inside when 0 <= r_a < (float)dim_a on all three axes.  Only inside
      samples are fetched.
   4. Sampling: NEAREST reads voxel ((int)r_x, (int)r_y, (int)r_z).  TRILINEAR: GL's linear rule at the continuous voxel
      coordinates (u, v, w) = q, taps clamped to the edge, lerps x then y then z (the isosurface mode's sampler).  s_k is the
      raw stored value, before the window.
   5. Reduction over the inside samples in increasing k: VR_SLAB_MIP keeps the max (replacing on s > m), VR_SLAB_MINIP the min
      (replacing on s < m), VR_SLAB_MEAN acc = acc + s from 0.0f, then value = acc / (float)cnt.  n = 1: the three agree.
   6. Output: cnt = 0: (0, 0, 0, 0), the background of every mode.  Else v = the composite mode's window of value (max == min:
      0); without a transfer function (v, v, v, 1), with one (rgb of the LUT at the composite mode's index rule, 1).
   7. vr_read_reslice_values: value - 1000.0f for 16-bit data under VR_QUIRK_U16_OFFSET (the window's units, HU), value
      otherwise; the quiet NaN 0x7fc00000 where cnt = 0.
   8. vr_count_samples: cnt.
   Row ranges, stripes, compact external targets, VR_QUIRK_TRUNC_GRID and volumes beyond 32-bit offsets apply.  Without a
   transfer function it is a grey mode (VR_FB_GREYALPHA32F targets, a vr_group's (grey, alpha) gather).  vr_set_skip_empty
   has no effect; vr_get_launch_choice is 0 after a reslice frame and the measured launch choices are untouched.
   VR_E_INVALID for an unknown mode, n outside 1..1024, a non-finite geometry float or while the isosurface mode is on (and
   vr_set_isosurface(h, 1, ...) is refused while this mode is on); enable = 0 ignores the other arguments (may be NULL) and
   always succeeds. */
enum { VR_SLAB_MIP = 0, VR_SLAB_MINIP = 1, VR_SLAB_MEAN = 2 };
int vr_set_reslice(vr_handle h, int enable, const float geom12[12], int slab_mode, int slab_samples);
/* the last reslice frame's values: one float per pixel of the colour target, indexed like it (as vr_read_depth); pixels that
   frame did not render keep earlier values (NaN initially).  VR_E_INVALID before the first reslice frame. */
int vr_read_reslice_values(vr_handle h, float *values, size_t n_floats);
/* Gradient-lit compositing, "shade" (no reference equivalent): the composite image with each visible sample's colour lit by
   the data's gradient and the isosurface mode's two-sided headlight.  An option of the composite mode only: with the MIP
   switch on frames are the MIP frames bit for bit, and while the isosurface or reslice mode is on that mode renders as
   before; the shading state is kept throughout (neither mode refuses it, it refuses neither).  Default off; initial
   coefficients 0.15, 0.65, 0.2, shininess 16 (the isosurface mode's constants).  Per pixel, each step one correctly rounded
   fp32 operation in the order given (nothing contracted; the only fused operations are TRILINEAR's lerps, as in the other
   modes):
   1. March, window, classification: exactly the composite mode's -- the ray, box entry, p0, the composite step, both
      VR_ACCUM_* modes, the view mapping, the loop-top test including dest.a >= 0.95, max_steps, the window, the grey ramp or
      the transfer function's index rule; then a = src.a * alpha_scale.
   2. A sample with a != 0 is shaded (steps 3, 4).  One with a == 0 adds the same bits shaded or not (finite rgb x 0): no
      gradient is taken for it.
   3. Normal at the sample position q_i: the isosurface mode's step 4 with h = q_i -- NEAREST at the sample's own voxel indices
      +- 1, TRILINEAR at the continuous coordinates u +- 1, v +- 1, w +- 1 around the sample, clamped; the view's box-space
      mapping; N = v * (1 / sqrt(dot)); dot = 0: N = -dir.
   4. Headlight: the isosurface mode's step 5 -- d made non-negative; spec = d^shininess by log2(shininess) squarings
      (shininess 1: spec = d); lit = ambient + diffuse * d (the product first); per r, g, b: c' = min(c * lit + specular * spec, 1).
   5. Compositing: exactly the composite mode's with c' in place of the classified rgb: src.rgb *= a, om = 1 - dest.a,
      dest += src * om, and the dest.a > 0.99 break.
   Consequences: alpha and vr_count_samples (gradient taps are not counted) are those of the unshaded composite frame;
   (1, 0, 0, any) gives the unshaded composite frame bit for bit (LUT entries and grey values lie in [0, 1]); without a
   transfer function r == g == b, so it is a grey mode (VR_FB_GREYALPHA32F targets, a vr_group's (grey, alpha) gather).
   vr_set_skip_empty applies with the composite mode's dilated 8^3 cell-max grid and threshold rule (NEAREST: every value up
   to the threshold has a == 0; TRILINEAR: the table's whole leading zero-alpha run): skipped samples have a == 0, so frames
   and counts are the same bits either way.  Row ranges, stripes, compact and grey-alpha external targets, VR_QUIRK_TRUNC_GRID,
   volumes beyond 32-bit offsets, vr_render_async and vr_group members apply.  A shaded frame explores, settles and evicts
   nothing in the measured launch choices; vr_get_launch_choice is 0 after it.
   VR_E_INVALID for a coefficient that is non-finite or < 0, or a shininess outside 1, 2, 4, ..., 128; a refused call changes
   nothing.  enable = 0 ignores the other arguments and always succeeds. */
int vr_set_shading(vr_handle h, int enable, float ambient, float diffuse, float specular, int shininess);
/* the shading state (any pointer may be NULL) */
int vr_get_shading(vr_handle h, int *enable, float *ambient, float *diffuse, float *specular, int *shininess);
/* Gaussian smoothing of the resident volume, computed on the device (no reference equivalent; the step VTK, ParaView and
   3D Slicer put in front of surface extraction and shading): the isosurface normal, the shading gradient and the resliced
   values are differences of neighbouring voxels, which voxel noise dominates.  Separable, one sigma per volume axis in
   voxels (x the fastest axis).  Each step is one correctly rounded operation in the order given:
   1. Source: always the volume AS LOADED, never an earlier smoothing result, so a sigma slider does not accumulate.  While a
      smoothed volume is in use the handle keeps the loaded one resident beside it.  (0, 0, 0) drops the smoothed volume and
      renders the loaded one again, bit for bit as before the first call.  Loading, generating or reading a new volume
      resets the state to (0, 0, 0).
   2. Arguments: each sigma finite and 0 <= sigma <= 8; anything else is VR_E_INVALID and changes nothing.  sigma_a == 0: no
      pass along axis a (the exact identity).  Without a volume: VR_E_INVALID (as vr_read_volume); a host-only handle:
      VR_E_NO_DEVICE; a device allocation that fails: VR_E_NOMEM, and the handle keeps rendering what it rendered before.
   3. Weights (vr_smooth_weights computes them, for the kernels' host side too): r = ceil(3 * sigma), at most 24;
      g_t = exp(-t*t / (2 * sigma*sigma)) in double for t = -r .. r; sum = their sum in double, in increasing t;
      w_t = (float)(g_t / sum).  *radius = r (may be NULL) and 2r + 1 floats are written; capacity < 2r + 1, a NULL w or a
      sigma outside (0, 8]: VR_E_INVALID.
   4. One pass along axis a over fp32 input `in`: acc = 0.0f; for t = -r .. r in increasing order
      acc = acc + w_t * in[clamp(i_a + t, 0, dim_a - 1)] -- the product rounded, then the sum, nothing contracted into an fma.
      Edges clamp, like the sampler.
   5. Order: x, then y, then z.  The first pass reads (float)voxel; intermediates stay fp32, with no rounding to integers
      between passes.
   6. Store: v = the last pass's fp32 value rounded half to even, clamped to [0, 255] or [0, 65535], in the loaded volume's
      type and layout.
   Kept: the window (vr_get_window), the camera, view, filter, transfer function, the modes and the launch stream; no message
   is queued.  vr_get_dataset_range, vr_histogram, vr_read_volume and vr_measure_stream_read report the volume being
   rendered, i.e. the smoothed one; vr_get_dims is unchanged.  Everything derived from voxel values is rebuilt or invalidated
   as a fresh load leaves it: the exact range that gates the 12-bit packed copy, that copy and every apron copy, the skip
   grid and its minimum, the tile order under skipping (the measured launch choices are keyed by the configuration, never by
   voxel values: a load keeps them and so does this call; whichever candidate runs, the frame is the same bits).  The
   smoothed volume has the loaded one's storage (zeroed brick padding, the slack slab).  vr_set_layout afterwards re-lays
   out both volumes and does not recompute the smoothing.  In vr_get_resident_bytes `volume` is the rendered volume and the
   kept loaded one counts under `other`: it is not an optional copy and vr_set_copy_budget never frees it.  Members of a
   vr_group are ordinary handles: smooth every member with the same values.
   Intermediates are fp32 planes on the device, freed before the call returns: the whole volume's where one buffer fits
   the workspace bound (vr_set_smoothing_workspace: bytes of one of the two buffers; 0, the default: 2 GiB or what the
   device has free), else z slabs of it, so device memory does not bound the volume size; the voxels are the same bits for
   every slab size.  A bound below one slab's planes (2 r_z + 1) gives VR_E_NOMEM. */
int vr_smooth_volume(vr_handle h, float sigma_x, float sigma_y, float sigma_z);
int vr_get_smoothing(vr_handle h, float sigma3[3]);                /* (0, 0, 0): not smoothed */
int vr_smooth_weights(float sigma, float *w, int capacity, int *radius);   /* host only, no handle */
int vr_set_smoothing_workspace(vr_handle h, uint64_t bytes);
/* measurement aid: HIP-event time, in ms, of the passes of the last vr_smooth_volume that ran any (first launch to last,
   every slab; allocations, the range scan and host work excluded); 0 before the first and after a call that ran none */
int vr_get_smoothing_ms(vr_handle h, float *ms);
/* Grey-level morphology and the median of the resident volume, computed on the device (no reference equivalent; 3D Slicer's
   Segment Editor "Smoothing" -- median, opening, closing -- and "Margin" -- grow, shrink; VTK's vtkImageContinuousErode3D,
   vtkImageContinuousDilate3D and vtkImageMedian3D): what goes between a threshold and the components.  A median removes
   salt-and-pepper voxels, which a Gaussian smears into the surface, and keeps edges; an opening cuts thin bridges and a closing
   fills pinholes without moving the iso level.  All five are rank filters on integers, so the result is defined bit for bit
   with no rounding rule:
   1. Window.  The window of voxel (i, j, k) is the box of (2rx+1)(2ry+1)(2rz+1) values
      in[clamp(i+a, 0, nx-1), clamp(j+b, 0, ny-1), clamp(k+c, 0, nz-1)] for |a| <= rx, |b| <= ry, |c| <= rz: edges clamp like
      the sampler and the Gaussian; x is the fastest axis; the values are the raw stored voxels compared as UNSIGNED integers.
   2. Single operations.  VR_RANK_ERODE is the window's minimum, VR_RANK_DILATE its maximum, VR_RANK_MEDIAN the element at
      0-based position (n-1)/2 of the window's n values in ascending order; n is always odd, so nothing is averaged.
   3. Two-stage operations.  VR_RANK_OPEN is ERODE, then DILATE of that result with the same box; VR_RANK_CLOSE is DILATE, then
      ERODE.  The second stage clamps at the edges of the first stage's OUTPUT.
   4. Arguments.  op in 0 .. 5; every radius in 0 .. 8 for ERODE, DILATE, OPEN and CLOSE, in 0 .. 1 for MEDIAN (windows from
      3x1x1 to 3x3x3; rz = 0 is the 3x3 in-plane median of anisotropic CT); anything else is VR_E_INVALID and changes nothing.
      VR_RANK_OFF, or all radii 0, is the identity, and the state then reads back (VR_RANK_OFF, 0, 0, 0).  Without a volume:
      VR_E_INVALID; a host-only handle: VR_E_NO_DEVICE; a device allocation that fails: VR_E_NOMEM -- as vr_smooth_volume, and
      after a failure the handle keeps rendering what it rendered before.
   5. Composition with the Gaussian.  The volume being rendered is always G(R(loaded)): R the rank filter in force, G
      vr_smooth_volume's sigmas in force, applied by its own definition to R's voxels.  Either call recomputes from the volume
      AS LOADED: nothing accumulates and the order of the two calls does not matter.  (VR_RANK_OFF) together with (0, 0, 0)
      renders the loaded volume again, bit for bit.  With the rank filter off vr_smooth_volume is exactly what it is without
      this call.  A load, vr_set_volume and vr_generate_synthetic reset both.
   6. Everything else follows vr_smooth_volume.  Kept: the window, camera, modes, transfer function, the launch stream, the
      launch choices and the resident mesh.  Rebuilt or invalidated as a fresh load leaves them: both ranges, the packed copy,
      the apron copies, the skip grid, the tile order under skipping and the ray stream.  The labelling is dropped.
      vr_read_volume, vr_histogram and vr_get_dataset_range report the rendered volume.  The loaded volume counts under
      `other` in vr_get_resident_bytes, and vr_set_layout re-lays out both volumes without recomputing.
   7. Memory.  Intermediates are voxel-typed whole volumes in the loaded volume's type and layout -- no fp32 copy, no z slabs: a
      buffer is the volume's own size -- and are freed before the call returns.  Minimum and maximum are separable (one pass per
      axis with r > 0, in the order x, y, z; OPEN and CLOSE run that twice), the median is one pass.  A call needs up to three
      volumes' worth of free device memory (the result; one intermediate when there is more than one pass; R's voxels while a
      Gaussian is in force, next to that Gaussian's own workspace); failure to get it is VR_E_NOMEM. */
#define VR_RANK_OFF 0
#define VR_RANK_ERODE 1     /* minimum over the box */
#define VR_RANK_DILATE 2    /* maximum over the box */
#define VR_RANK_OPEN 3      /* ERODE, then DILATE of that result, same box */
#define VR_RANK_CLOSE 4     /* DILATE, then ERODE of that result, same box */
#define VR_RANK_MEDIAN 5
int vr_rank_filter_volume(vr_handle h, int op, int rx, int ry, int rz);
int vr_get_rank_filter(vr_handle h, int *op, int r3[3]);           /* any pointer may be NULL */
/* measurement aid, like vr_get_smoothing_ms: HIP-event time, in ms, of the passes of the last rank filter that ran any (first
   launch to last; allocations, a Gaussian that followed, the range scan and host work excluded); 0 before the first */
int vr_get_rank_filter_ms(vr_handle h, float *ms);
/* Extraction of the isosurface s = iso of the resident volume -- the one being rendered, i.e. the smoothed one after
   vr_smooth_volume -- as a watertight indexed triangle mesh, computed on the device (no reference equivalent): positions in
   the units of vr_get_dims' spacing, unit normals, uint32 triangle indices.  Marching tetrahedra on the Kuhn (six-tetrahedra)
   split of every voxel cell: no ambiguous cases, so the surface is edge-manifold by construction.  The surface is open where
   it meets the volume's boundary; caps are out of scope.  Every step is one correctly rounded fp32 operation in the order
   given, nothing contracted:
   1. Lattice: voxel (i, j, k) is a lattice point, x the fastest axis.  A cell is the cube between (i, j, k) and
      (i+1, j+1, k+1): (nx-1)(ny-1)(nz-1) cells.  Any dimension below 2: no cells, the mesh is empty (0 vertices, 0 triangles)
      and the call succeeds.
   2. Values: s = (float) of the raw stored voxel.  iso_s = float(iso_value + 1000) for 16-bit data under
      VR_QUIRK_U16_OFFSET, float(iso_value) otherwise (vr_set_isosurface's rule: both show the same surface).  A voxel is
      INSIDE when s >= iso_s.
   3. Edges: the seven directions e_0 .. e_6 = (1,0,0), (0,1,0), (0,0,1), (1,1,0), (1,0,1), (0,1,1), (1,1,1).  Edge (A, d)
      runs from voxel A to B = A + e_d and exists when B lies in the volume.  It carries a vertex when exactly one of A and B
      is inside.
   4. Vertex: f = (iso_s - s_A) / (s_B - s_A) (two subtractions, one division; f lies in [0, 1]).  Per axis a:
      p_a = ((float)A_a + f) * spacing_a where e_d has a 1 on that axis, (float)A_a * spacing_a where it has a 0: voxel
      (0,0,0)'s centre is the origin.  f = 0 (s_A == iso_s) makes vertices coincide; the zero-area triangles are kept.
   5. Normal: g(V)_a = S(min(V_a+1, dim_a-1)) - S(max(V_a-1, 0)) at voxel indices (the isosurface mode's NEAREST gradient);
      G_a = g(A)_a + f * (g(B)_a - g(A)_a) (difference, product, sum); H_a = G_a / spacing_a; v = -H;
      dot = (v_z*v_z + v_y*v_y) + v_x*v_x; N = v * (1.0f / sqrtf(dot)), (0,0,0) when dot == 0.  It points to lower values,
      out of bright objects.
   6. Vertex order: by the owner voxel A's linear index i + nx*(j + ny*k), then by d.
   7. Tetrahedra: for the axis permutations pi in the order xyz, xzy, yxz, yzx, zxy, zyx, tetrahedron t has the corners
      c_0 = (0,0,0), c_1 = c_0 + e_pi1, c_2 = c_1 + e_pi2, c_3 = (1,1,1) relative to the cell.  Every tetrahedron edge
      c_n -> c_m (n < m) is edge (cell + c_n, direction c_m - c_n) of step 3: vertices are shared between tetrahedra and cells.
   8. Cases: m = the mask of inside corners (bit n: c_n); I, O = the inside, outside corners in ascending order; xy = the
      vertex on the tetrahedron edge between corners x and y.  |I| = 1, a = I_0: triangle (aO_0, aO_1, aO_2).  |I| = 3,
      a = O_0: (aI_0, aI_1, aI_2).  |I| = 2, I = (a, b), O = (c, d): (ac, ad, bd) and (ac, bd, bc).  m = 0, 15: none.
   9. Winding: the second and third vertex of every triangle of an entry (t, m) are swapped when, with the vertices at the
      edge midpoints in lattice coordinates, (v_1 - v_0) x (v_2 - v_0) . (mean of O - mean of I) < 0 for its first triangle:
      the front face, counter-clockwise, is seen from the outside.  Check value: the even permutations xyz, yzx, zxy swap
      exactly m in {2, 5, 8, 10, 11, 14}, the odd ones the other eight cases.
   10. Triangle order: by the cell's linear index i + (nx-1)*(j + (ny-1)*k), then t, then the order within the case.
   The mesh is a snapshot on the device: it stays valid until the next extraction, vr_free_mesh or vr_destroy, survives
   loading or smoothing another volume, and counts under `other` in vr_get_resident_bytes.  An extraction changes no
   rendering state (window, modes, launch choices, copies, stream) and queues no message on success.  Errors: no volume:
   VR_E_INVALID; a host-only handle: VR_E_NO_DEVICE; more than 2^32 - 1 vertices or triangles: VR_E_INVALID and a message for
   vr_take_message; a device allocation that fails: VR_E_NOMEM; after any of them the previous mesh is still there.
   vr_get_mesh_info, vr_read_mesh and vr_save_mesh before the first mesh, a capacity (in vertices, triangles) that is too
   small, an unknown extension: VR_E_INVALID.  n_vertices, n_triangles and any pointer of vr_read_mesh may be NULL.
   vr_save_mesh: ext "stl" = binary STL (80-byte header that does not begin with `solid`, uint32 count, 50 bytes a triangle;
   the facet normal is the unit cross product of the stored positions computed in double, (0,0,0) for a zero-area triangle;
   attribute word 0); "ply" = binary_little_endian 1.0, vertex properties x y z nx ny nz as float, faces uchar uint.
   Work arrays (9 bytes a voxel) are bounded by vr_set_mesh_workspace (0, the default: 2 GiB or what the device has free):
   the extraction runs in z slabs that fit, and the mesh is the same bytes for every slab size and on every run.  A bound
   below two planes gives VR_E_NOMEM. */
int vr_extract_isosurface(vr_handle h, int32_t iso_value, uint64_t *n_vertices, uint64_t *n_triangles);
int vr_get_mesh_info(vr_handle h, int32_t *iso_value, uint64_t *n_vertices, uint64_t *n_triangles);
int vr_read_mesh(vr_handle h, float *positions, float *normals, uint32_t *triangles,
                 uint64_t vertex_capacity, uint64_t triangle_capacity);
int vr_save_mesh(vr_handle h, const char *path, const char *ext);
int vr_free_mesh(vr_handle h);
int vr_set_mesh_workspace(vr_handle h, uint64_t bytes);
/* measurement aid: HIP-event time, in ms, of the kernels of the last successful vr_extract_isosurface (the counting pass plus
   the emitting pass; allocations and host work excluded); 0 before the first */
int vr_get_mesh_ms(vr_handle h, float *ms);
/* Connected components of the inside voxels, labelled on the device, and the extraction of only the selected ones (no
   reference equivalent; VTK's connectivity filter, 3D Slicer's "Islands", ParaView's "Extract largest region"): at a bone
   threshold a CT gives one skeleton, the scanner table and tens of thousands of specks; this keeps the largest pieces or drops
   the small ones before a single triangle is written.
   1. Inside: as step 2 of the extraction: s = (float) of the raw stored voxel of the volume being rendered (the smoothed one
      after vr_smooth_volume); iso_s = float(iso_value + 1000) for 16-bit data under VR_QUIRK_U16_OFFSET, float(iso_value)
      otherwise.  A voxel is INSIDE when s >= iso_s.
   2. Adjacency: inside voxels A and B = A + e_d are adjacent for d = 0 .. 6, the extraction's seven directions (1,0,0), (0,1,0),
      (0,0,1), (1,1,0), (1,0,1), (0,1,1), (1,1,1): with their opposites a 14-neighbourhood.  The other 12 of the 26 neighbours --
      (1,-1,0), (1,0,-1), (0,1,-1), (1,1,-1), (1,-1,1), (-1,1,1) and their opposites -- are NOT adjacent.  A component is a class
      of the transitive closure.  Why these: every edge of a Kuhn tetrahedron is one of the seven directions, so the inside
      corners of any tetrahedron lie in one component, an edge that carries a vertex has exactly one inside end, and every
      triangle of the mesh belongs to exactly one component.
   3. Numbering: a component's FIRST VOXEL is its voxel of lowest linear index i + nx*(j + ny*k).  Components are numbered
      1 .. n by ascending first voxel; outside voxels have label 0.  The numbering, and so every output, is the same bytes on
      every run.  More than 2^32 - 2 components: VR_E_INVALID and a message for vr_take_message, the previous labelling kept.
   4. Record per component (vr_read_components; entry label - 1; any pointer may be NULL; a capacity below n: VR_E_INVALID):
      voxels (uint64), first_voxel (uint64 linear index), bbox (six int32: lo x, y, z, hi x, y, z, inclusive), selected (uint8).
   5. Labels: one uint32 per voxel, x fastest, in linear order whatever the volume's layout (vr_read_labels: n_voxels at least
      nx*ny*nz; vr_component_at: one voxel's).  They stay on the device and count under `other` in vr_get_resident_bytes.
      Unlike the mesh the labelling is not a product: it belongs to the voxels and is dropped when the rendered voxels change --
      a load, vr_set_volume, vr_generate_synthetic, vr_smooth_volume -- and by vr_free_components.  It survives vr_set_layout,
      the window, the camera, the modes and vr_set_quirks, because it keeps its own iso_s.
   6. Selection: after labelling every component is selected.  vr_select_components(min_voxels, keep_largest): a component is
      selected when voxels >= min_voxels and, when keep_largest > 0, it is among the keep_largest first in the order (voxels
      descending, label ascending).  vr_select_component_list selects exactly the listed labels (n = 0: none); a label of 0 or
      above n: VR_E_INVALID and nothing changes.  Selection is host logic on the records; the per-voxel work stays on the device.
   7. Filtered extraction, vr_extract_components: the mesh of vr_extract_isosurface at the labelling's iso value (and iso_s)
      with step 2's INSIDE replaced by "INSIDE and its component is selected".  Everything else is unchanged: s, f, positions,
      gradients and normals from the raw voxels, the vertex and triangle order, the z slabs under vr_set_mesh_workspace, the
      2^32 - 1 limits and their errors.  It replaces the handle's mesh: vr_get_mesh_info (which reports the labelling's iso
      value), vr_read_mesh, vr_save_mesh, vr_free_mesh and vr_get_mesh_ms serve it.  Consequences: with every component selected
      it is vr_extract_isosurface's mesh byte for byte; otherwise it is that mesh's sub-mesh -- the kept vertices and triangles
      in their order, the indices renumbered -- and no other byte changes.  (Zeroing the removed voxels and extracting again is
      NOT the same: it changes the normals of kept vertices beside removed voxels, whose central differences read them.)
      Nothing selected: the empty mesh, VR_OK.  Without a labelling: VR_E_INVALID.
   8. Errors, as the extraction's: no volume: VR_E_INVALID; a host-only handle: VR_E_NO_DEVICE; a device allocation that fails:
      VR_E_NOMEM; a kernel whose union-find loop hits its iteration cap (a defect, not an input): VR_E_HIP; after any of them
      the previous labelling and mesh are still there.  The queries before the first labelling: VR_E_INVALID.  Labelling
      changes no rendering state and queues no message on success.
   Memory: the labels are whole-volume, with no slab path: 4 bytes a voxel, plus 8 bytes a voxel of parents while labelling a
   volume of 2^32 - 1 voxels or more (1024^3: 4 GiB; 2048^3: 96 GiB while labelling, 32 GiB afterwards), plus 1/4 byte a voxel
   of root bits and counts; vr_extract_components adds 1/8 byte a voxel for the selection.  VR_E_NOMEM where it does not fit.
   vr_set_component_index_bits: aid for tests: 0 (default) automatic, 32, 64 = the parents' width for the next labelling (32 on
   a volume it cannot number: that labelling gives VR_E_INVALID); other values: VR_E_INVALID. */
int vr_label_components(vr_handle h, int32_t iso_value, uint64_t *n_components);
int vr_get_components_info(vr_handle h, int32_t *iso_value, uint64_t *n_components, uint64_t *n_inside, uint64_t *n_selected);
int vr_read_components(vr_handle h, uint64_t *voxels, uint64_t *first_voxel, int32_t *bbox6, uint8_t *selected, uint64_t capacity);
int vr_read_labels(vr_handle h, uint32_t *labels, uint64_t n_voxels);
int vr_component_at(vr_handle h, int i, int j, int k, uint32_t *label);
int vr_select_components(vr_handle h, uint64_t min_voxels, uint64_t keep_largest, uint64_t *n_selected);
int vr_select_component_list(vr_handle h, const uint32_t *labels, uint64_t n, uint64_t *n_selected);
int vr_extract_components(vr_handle h, uint64_t *n_vertices, uint64_t *n_triangles);
int vr_free_components(vr_handle h);
int vr_set_component_index_bits(vr_handle h, int bits);
/* measurement aid: HIP-event time, in ms, of the kernels of the last successful vr_label_components (tile pass, seam pass,
   flatten, scan, labels, records; allocations, read-backs and host work excluded); 0 before the first */
int vr_get_components_ms(vr_handle h, float *ms);
/* Simplification of the resident mesh by vertex clustering, computed on the device (no reference equivalent; Rossignac and
   Borrel's clustering, VTK's vtkQuadricClustering with an input vertex as the representative): vr_simplify_mesh replaces the
   handle's mesh, whether vr_extract_isosurface or vr_extract_components made it, by its simplification.  vr_get_mesh_info
   (the iso value is unchanged), vr_read_mesh, vr_save_mesh, vr_free_mesh and `other` of vr_get_resident_bytes then serve the
   new mesh.  Every fp32 step is one correctly rounded operation in the order given, nothing contracted:
   1. Input: the resident mesh, V vertices (positions in the spacing's units, all >= 0, and normals) and T triangles; `cell`,
      the edge length of the cubic clustering cells in the same units.  The grid is anchored at the origin, voxel (0,0,0)'s centre.
   2. Cell of a vertex: per axis q_a = p_a / cell (one division) and c_a = (int)floorf(q_a).  A q_a that is not below 2097152.0f
      (2^21) -- or is negative or NaN, which no extraction produces -- is an error: VR_E_INVALID, a message for vr_take_message,
      the mesh untouched.  Two vertices are in the same cluster when their three c_a are equal.
   3. Representative: centre_a = ((float)c_a + 0.5f) * cell (the sum is exact, the product rounded once); d_a = p_a - centre_a;
      dist = (d_z*d_z + d_y*d_y) + d_x*d_x.  A cluster's representative is its vertex of smallest dist, ties going to the lowest
      vertex index (so coincident vertices, which the extraction produces where s_A == iso_s, resolve by index).  It is an input
      vertex: it keeps its position and normal bits and stays on the isosurface.  Nothing is averaged.
   4. Triangles: every index is replaced by its cluster's representative.  A triangle with two equal indices is dropped.  Of the
      remaining triangles with the same unordered vertex set only the one of lowest input index is kept, with its own
      orientation.  Kept triangles stay in input order.
   5. Vertices: only representatives that a kept triangle references are kept, in ascending input index, renumbered
      0 .. V'-1: the output vertices are rows of the input's position and normal arrays in their order, as with
      vr_extract_components' sub-mesh.
   6. Consequences: every output vertex is referenced; no two output vertices share a cell; every triangle has three different
      indices and no two triangles have the same vertex set; simplifying the result again with the same cell gives the same
      bytes; a cell larger than the mesh's extent gives the empty mesh with VR_OK; the empty mesh simplifies to the empty mesh.
      Closedness and edge-manifoldness are NOT preserved (as with VTK's filter): a thin sheet may collapse onto itself, a
      tunnel may close, an edge may end up with one or with more than two triangles.
   7. State: the new arrays are built first and swapped in at the end; after any error the previous mesh is still there.  The
      call changes no rendering state (window, modes, copies, launch choices, stream), keeps the labelling and queues no message
      on success.  Work arrays live on the device and are freed before it returns: while the vertices are clustered 40 bytes a
      vertex (keys and indices before and after the sort, distances, cluster numbers, representatives, run heads) plus 8 bytes a
      cluster, then 12 bytes a vertex and 48 bytes a triangle (the triples before, between and after their two sorts, the two
      orders, the kept flags) plus 4 bytes a cluster; in both stretches rocPRIM's sort scratch on top, which is at most one more
      copy of the keys and values being sorted (12 bytes an element).  VR_E_NOMEM where that does not fit.
   8. Errors, checked in this order: a host-only handle: VR_E_NO_DEVICE; cell not finite, not a normal number or <= 0:
      VR_E_INVALID; no mesh: VR_E_INVALID; step 2's refusal; a device allocation that fails: VR_E_NOMEM.  n_vertices and
      n_triangles may be NULL.
   9. vr_get_mesh_simplification (any pointer may be NULL): after an extraction cell = 0 and the mesh's own counts; after a
      simplification that call's cell and the counts of the mesh it was given; before the first mesh and after vr_free_mesh:
      VR_E_INVALID.
   10. vr_get_simplify_ms: measurement aid: HIP-event time, in ms, of the kernels and device sorts of the last successful
      vr_simplify_mesh (allocations, read-backs and host work excluded); 0 before the first and after one of an empty mesh. */
int vr_simplify_mesh(vr_handle h, float cell, uint64_t *n_vertices, uint64_t *n_triangles);
int vr_get_mesh_simplification(vr_handle h, float *cell, uint64_t *source_vertices, uint64_t *source_triangles);
int vr_get_simplify_ms(vr_handle h, float *ms);
/* Smoothing of the resident mesh, computed on the device (no reference equivalent; Taubin's lambda|mu filter, the step VTK's
   vtkSmoothPolyDataFilter / vtkWindowedSincPolyDataFilter and 3D Slicer's "Smoothing factor" put last): vr_smooth_mesh replaces
   the positions and normals of the handle's mesh, whichever extraction or simplification made it, by their smoothed values.  The
   triangles, V and T are unchanged; vr_get_mesh_info, vr_read_mesh, vr_save_mesh and vr_free_mesh serve the result.  Every fp32
   step is one correctly rounded operation in the order given, nothing contracted:
   1. Input: the resident mesh, V vertices and T triangles; iterations, lambda, mu, fix_boundary.
   2. Graph: every triangle (a, b, c) contributes the directed pairs (a,b), (b,a), (b,c), (c,b), (c,a), (a,c).  Pairs with equal
      ends are ignored (no extraction or simplification produces them; the definition is total).  N(i) is the set of distinct j
      with a pair (i, j), k_i = |N(i)|.  The multiplicity of {i, j} is the number of pairs (i, j): the number of triangles that
      contain the edge.  The graph is built on indices, not positions: coincident vertices, which the extraction produces where
      s_A == iso_s, are different vertices.
   3. Fixed vertices: with fix_boundary != 0 a vertex is FIXED when it is an end of an edge of multiplicity exactly 1; with
      fix_boundary == 0 nothing is fixed.  A vertex with k_i = 0 never moves.  On an extracted mesh the fixed vertices are
      exactly those where the open surface meets the volume's boundary, so the cut stays planar; on a simplified mesh they are
      also the ends of edges that clustering left with one triangle.
   4. A step with factor phi is Jacobi: every vertex reads the positions from before the step.  For every vertex i that is not
      fixed and has k_i > 0, per axis a: acc = 0.0f; acc = acc + p_j,a over j in N(i) in ascending j; m = acc / (float)k_i (one
      division); d = m - p_i,a; p'_i,a = p_i,a + phi * d (the product, then the sum).  All other vertices keep their bits.
   5. An iteration: a step with phi = lambda, then a step with phi = mu; the mu step is skipped when mu == 0 (plain Laplacian
      smoothing).  `iterations` iterations are run.
   6. Normals: recomputed from the result (the stored gradient normals belong to the old positions).  Per triangle t with corners
      p0, p1, p2: u = p1 - p0, w = p2 - p0, c_x = u_y*w_z - u_z*w_y and c_y, c_z cyclically (each two products and one
      subtraction).  Per vertex: S = (0, 0, 0); S_a = S_a + c(t)_a over every (t, corner) that references the vertex, in ascending
      (t, corner); dot = (S_z*S_z + S_y*S_y) + S_x*S_x; N = S * (1.0f / sqrtf(dot)), and (0, 0, 0) when dot == 0 -- the
      extraction's step 5 normalisation.  The front face is counter-clockwise seen from outside, so N points the way the old
      normals did.  A vertex no triangle references gets (0, 0, 0).
   7. iterations == 0: VR_OK, the mesh keeps every byte including its normals, nothing is launched.
   8. Consequences: smoothing n then m iterations with the same lambda, mu and flag gives the bytes of n + m iterations (the mesh
      is a product: unlike vr_smooth_volume, which always starts from the volume as loaded, calls accumulate); the triangles are
      untouched; fixed vertices keep their position bits.  A mu < 0 step can push a coordinate below 0 near the origin, and
      vr_simplify_mesh refuses such a mesh by its own step 2: the order is simplify, then smooth.
   9. Parameters and errors, checked in this order: a host-only handle: VR_E_NO_DEVICE; iterations outside [0, 1000], lambda not
      finite or not in (0, 1], mu not finite or not in [-2, 0]: VR_E_INVALID; no mesh: VR_E_INVALID; 6*T > 2^32 - 1 (pair numbers
      and row offsets are 32-bit): VR_E_INVALID and a message for vr_take_message; a device allocation that fails: VR_E_NOMEM.
      The new arrays are swapped in at the very end: after any error the previous mesh is still there.  No rendering state
      changes (window, modes, copies, launch choices, stream), the labelling is kept and success queues no message.  The empty
      mesh smooths to the empty mesh.
   10. vr_get_mesh_smoothing (any pointer may be NULL): the arguments of the last successful vr_smooth_mesh on this mesh and its
      number of fixed vertices (0 where that call launched nothing: iterations == 0 or the empty mesh); iterations 0 and the rest
      0 after any extraction or simplification -- a new mesh is unsmoothed; before the first mesh and after vr_free_mesh:
      VR_E_INVALID.  vr_get_mesh_simplification and vr_get_mesh_info are unaffected.
   11. vr_get_mesh_smooth_ms: measurement aid: HIP-event times, in ms, of the last successful vr_smooth_mesh, split into building
      the graph (pairs, sort, rows, fixed vertices) and everything after it (steps and normals); allocations, read-backs and
      host work excluded; 0 before the first call and after one that launched nothing.  Either pointer may be NULL, both:
      VR_E_INVALID.
   Memory: work arrays live on the device and are freed before the call returns.  While the graph is built 120 bytes a triangle
   (the six 64-bit pairs before and after their sort, their run heads) plus 12 bytes a vertex (rows, fixed flags) plus 4 bytes
   a distinct pair (3 T on a closed manifold, at most 6 T); during the steps 32 bytes a vertex (rows, two more copies of the
   positions) plus the neighbours; for the normals 16 bytes a triangle of face vectors and 48 of corners before and after
   their sort, and 32 bytes a vertex (the corner rows, the new positions and normals); rocPRIM's sort scratch on top, at most
   one more copy of what is being sorted.  VR_E_NOMEM where that does not fit. */
int vr_smooth_mesh(vr_handle h, int iterations, float lambda, float mu, int fix_boundary);
int vr_get_mesh_smoothing(vr_handle h, int *iterations, float *lambda, float *mu, int *fix_boundary, uint64_t *fixed_vertices);
int vr_get_mesh_smooth_ms(vr_handle h, float *build_ms, float *iterate_ms);
/* kernel selection: 0 = automatic (specialised kernels when the configuration allows; launches far from filling the
   chip -- fewer than 256 active 32x16 tiles, 1024 when the view is oblique to the volume axes -- use the 4-wavefront
   relay kernel; the fast kernel runs its software-pipelined batch loop unless alpha_scale >= 0.5),
   1 = always the generic line-by-line kernel (cross-check / debugging), 2 = the fast kernel with its
   plain loop: never the relay kernel, never the pipelined loop, 3 = automatic but always the relay kernel
   when the shape allows, 4 = retired (the NEAREST LDS-staged kernel of round 2 lost to the default kernels in every
   cell of the round-3 sweep, profiles/r03_work_model_sweep.txt, and was deleted; the value is refused),
   5 = the fast kernel with the pipelined loop, never the relay,
   6 = TRILINEAR on the LDS-staged kernel (the apron copy's bricks streamed into LDS, eight ds_read taps per
   sample; every mode incl. the transfer function; volumes beyond 4 GiB) wherever it is eligible,
   7 = that kernel with staging switched off: every tile takes the path of tiles whose brick layers do not fit LDS
   (pair loads from the apron copy, four samples' taps in flight) -- the cross-check of that path,
   8 / 9 = the LDS-staged kernel with one apron copy per major axis (so that every tile marches through layers of its
   own major axis with unit-stride DMA pieces) and the layer thickness chosen per tile: whole brick layers where they fit the tile's
   LDS ring, half layers (two voxels, 80-byte slots) where they do not -- 8 on 32x16-pixel tiles, 9 on 16x32-pixel tiles whose ring
   can also hold, per brick row, that row's own range (tiles whose bounding rectangles fit no other way: views near a body
   diagonal).  16-bit volumes; on 8-bit ones 8 runs as 6 and 9 as 6 on 16x32-pixel tiles.
   10 = the shape of 6 on 53 KiB of LDS: three workgroups per CU, six wavefronts per SIMD -- faster (6-13 %) wherever the tiles' brick
   layers fit (8-bit volumes, 16-bit ones up to ~512^3 or at 4K), slower where they do not; a candidate of the measured choice.
   11 = the LDS-staged kernel on 16x16-pixel tiles (four wavefronts, 40 KiB, four workgroups per CU; 16-bit volumes at oblique views
   with the per-axis copies and the thickness per tile): the first guess for volumes up to 640 voxels per axis, a candidate for
   launches that leave workgroup slots empty (round 6: cfg1 shape 0.138 -> 0.118 ms, cfg2 shape 0.402 -> 0.381).
   Frames are bit-identical under every variant. */
int vr_set_kernel_variant(vr_handle h, int variant);
/* 1 (default): under kernel variant 0 the launch is a MEASURED choice -- every candidate kernel of a configuration
   renders identical bits, so the first frames after a change of configuration (image, shard, volume, window, opacity,
   pose bucket; opacity and window width in coarse buckets, so a slider drag does not re-explore per frame) try the candidates
   in a shuffled order, twice each (HIP events on the launch stream, read without blocking), and the fastest is kept -- the
   heuristic's choice unless a rival is 2 % faster; a settled configuration is measured once more 96 frames later (clock
   ramp), entries are evicted least-recently-used first.  A configuration seen for fewer than three consecutive launches,
   and vr_set_autotune(0), get the heuristic's choice only.  Replaces round 2's tile-count thresholds; no reference equivalent (the reference has one shader). */
int vr_set_autotune(vr_handle h, int enable);
/* what the last launch ran as (for tests and tools; no reference equivalent): bit 0 relay kernel, bit 1 pipelined batch loop,
   bit 2 four-sample batches, bits 3..6 the LDS-staged trilinear kernel's shape (0 = not that kernel; the numbers of
   vr_set_kernel_variant 6 .. 11 minus 5), bit 8 (256): the measured choice is still EXPLORING this configuration -- the
   frame was a trial of one candidate (up to ~45 % slower than the settled choice), not the settled kernel */
int vr_get_launch_choice(vr_handle h);
/* The SETTLED entries of the measured choice as a flat blob, and back (round 6).  The reference dispatches one shader per frame and
   never tries anything (src/RendererCore.cpp:138-163); a handle that imports what another handle or an earlier process measured does
   the same for every configuration the blob knows: frame 1 runs on the settled kernel, no trial frames, no re-validation.
   vr_export_choices: *bytes = the size the blob needs (call with buf NULL to ask); it is written when capacity suffices, else VR_E_INVALID.
   vr_import_choices: *accepted = entries taken over; a blob measured on another device model or by another build of the library is
   well-formed but not trusted: 0 entries, VR_OK.  Malformed blobs: VR_E_INVALID. */
int vr_export_choices(vr_handle h, void *buf, size_t capacity, size_t *bytes);
int vr_import_choices(vr_handle h, const void *buf, size_t bytes, int *accepted);
/* 1 (default): when every voxel of a bricked 16-bit volume is <= 4095 (12-bit data) the
   specialised kernel gathers from a lossless 12-bit packed copy kept beside the volume (25 %
   fewer cache lines per frame; frames are bit-identical); 0: never.  Build-defined. */
int vr_set_pack12(vr_handle h, int enable);
/* bytes of the packed copy the last vr_render* gathered from (0: the launch used the volume as loaded) */
int vr_get_pack12_bytes(vr_handle h, size_t *bytes);
/* 1 (default): with VR_FILTER_TRILINEAR on the bricked layout the batched trilinear kernel gathers from an "apron"
   copy kept beside the volume -- every 4x4x4 brick stored as 5x4x4, i.e. with the x neighbours of its last column --
   so that the two x taps of a sample are one load for every lane (+25 % of the volume's bytes; 2.27 -> 1.8 ms on the
   1024^3 workload; frames are bit-identical); 0: never.  Build-defined, like the packed copy. */
int vr_set_trilinear_copy(vr_handle h, int enable);
/* bytes of the apron copy the last vr_render* gathered from (0: none) */
int vr_get_trilinear_copy_bytes(vr_handle h, size_t *bytes);
/* Device memory this handle holds right now (any pointer may be NULL): the volume as loaded (what the reference keeps
   in its 3-D texture, src/RendererCore.cpp:419); the optional speed copies built beside it (12-bit packed copy, apron
   copies: up to 0.75 + 3 x 1.25 volumes for a 16-bit volume viewed obliquely with TRILINEAR); everything else (targets,
   tables, skip grid, staging).  No reference equivalent (the GL driver owns the reference's memory). */
int vr_get_resident_bytes(vr_handle h, uint64_t *volume, uint64_t *copies, uint64_t *other);
/* Upper bound, in bytes, on the optional copies together.  VR_COPY_BUDGET_AUTO (default): a copy is built only while the
   device keeps max(1 GiB, a tenth of its memory) free after it, so that mandatory allocations that come later (skip grid,
   targets, a group's frame slots) still succeed.  0 = no copies at all.  Lowering the budget frees copies that no longer
   fit (per-axis aprons first, then the apron, then the packed copy); frames are bit-identical with or without any copy. */
#define VR_COPY_BUDGET_AUTO UINT64_MAX
int vr_set_copy_budget(vr_handle h, uint64_t bytes);
int vr_get_copy_budget(vr_handle h, uint64_t *bytes);
/* The ray-ordered sample stream of a still view (no reference equivalent; its GUI redraws continuously while only window,
   alpha and transfer-function sliders move).  Which voxel each sample of a NEAREST frame reads depends on the volume and the
   ray geometry only, so while camera, image, row range / stripes, volume, step and view switches stand still the voxels the
   shader's loop reads are kept in device memory in ray order, and frames are rendered by streaming them: every sample is
   still classified and composited with the frame's own window, alpha, transfer function and MIP setting, and frames are
   bit-identical to the gather kernels'.  Applies to the frames of the specialised NEAREST kernel with vr_set_skip_empty off.
   mode 0: never; 1 (default): from the 64th consecutive vr_render* of one geometry on, and never on a launch the measured
   launch choice wants timed; 2: build at the next eligible launch (tests and tools).  Any change of the geometry or of the
   rendered voxels makes the stream stale at once.  Building it runs two kernels and BLOCKS the calling thread once on an
   8-byte read-back (also inside vr_render_async).  The stream -- about 2 bytes (16-bit volumes) per sample of the frame plus
   padding, 1 GB for a 1024^3 volume at 1920x1080 -- is an optional copy: it counts under `copies` in vr_get_resident_bytes,
   obeys vr_set_copy_budget (the first copy freed) and is dropped with the voxels.  Its size depends on the view, so a stream
   that the budget or the device's memory refuses is refused for that geometry only -- not asked again while the geometry
   stands, asked again after any change of it.  vr_get_launch_choice is unaffected;
   vr_get_last_kernel_name reports raymarch_stream_kernel on replayed frames.  Other mode values: VR_E_INVALID. */
int vr_set_ray_stream(vr_handle h, int mode);
/* device bytes of the valid stream (samples, per-pixel counts, block offsets); 0: none */
int vr_get_ray_stream_bytes(vr_handle h, uint64_t *bytes);
/* how many streams this handle has built so far */
int vr_get_ray_stream_builds(vr_handle h, uint64_t *builds);
/* The stream's sample format.  A 16-bit volume whose exact range spans at most 4095 (12-bit CT data whatever its offset: the
   rule of the 12-bit packed volume copy, vr_set_pack12) can keep its stream as voxel - minimum in 12 bits, eight samples per
   12-byte load: a quarter fewer bytes resident, written by a build and read by every replayed frame, and the same frames bit
   for bit.  mode 0: never; 1 (default): when the stream's samples would take more than 256 MiB unpacked (the last-level
   cache of an MI355X: beyond it a replayed frame is an HBM stream); 2: whenever the volume allows.  8-bit volumes and wider
   ranges keep the unpacked stream under every mode.  A new mode makes the stream stale: the next eligible launch builds it
   again.  vr_get_last_kernel_name reports raymarch_stream12_kernel on frames replayed from a packed stream;
   vr_get_ray_stream_bytes is the real allocation either way.  Other mode values: VR_E_INVALID. */
int vr_set_ray_stream_pack(vr_handle h, int mode);
int vr_get_ray_stream_pack(vr_handle h, int *mode);
/* How a replayed frame classifies the grey ramp: arithmetically, or through a table of the window's entries in the CU's local
   memory whose reads are issued ahead of their use (for a fixed share of the samples: all of them, as built).  The table's
   entries are computed by the arithmetic path's own operations, so frames are the same bits.  Eligible: grey composite
   without a transfer function and plain MIP, a window of at most 4096 entries, and -- packed stream -- a window below 2^24 in
   magnitude.  mode 0: never; 1 (default): where eligible on a packed stream (vr_set_ray_stream_pack) whose samples take
   more than 256 MiB; 2: wherever eligible.  The stream is not rebuilt and
   vr_get_last_kernel_name is unchanged.  *used (may be null): 1 if the last replayed frame took the hybrid.  Other mode
   values: VR_E_INVALID. */
int vr_set_ray_stream_table(vr_handle h, int mode);
int vr_get_ray_stream_table(vr_handle h, int *mode, int *used);
/* 1-D transfer function (N3): n knots of (iso in 0..255, r,g,b,a); n = 0 restores the
   reference grey ramp.  Built with the natural cubic spline of src/CubicSpline.cpp. */
int vr_set_transfer_function(vr_handle h, const int32_t *iso, const float *rgba4, int n);
int vr_get_transfer_lut(vr_handle h, float lut_rgba[256 * 4]);
/* image-row shard rendered by this handle: global rows [row_begin,row_end); default all. */
int vr_set_row_range(vr_handle h, int row_begin, int row_end);
/* cyclic row stripes: this handle renders stripes s with s % count == index, each
   `stripe_rows` rows tall (count = 1 disables). */
int vr_set_row_stripes(vr_handle h, int stripe_rows, int index, int count);
/* compact = 1: the target holds only this handle's rows, local row r of the shard at
   offset r*fb_w (contiguous shard: r = row - row_begin; stripes: stripe-major).  Only
   meaningful with an external target; vr_local_rows() gives its height in rows. */
int vr_set_framebuffer_compact(vr_handle h, int compact);
/* format of an EXTERNAL target: VR_FB_RGBA32F (default, 4 floats per pixel) or
   VR_FB_GREYALPHA32F (2 floats per pixel: the grey value and alpha; in the reference's grey
   modes r == g == b bit for bit, so this is the same frame in half the bytes -- what a
   multi-GPU gather moves).  Rendering with a transfer function into it fails (VR_E_INVALID). */
#define VR_FB_RGBA32F 0
#define VR_FB_GREYALPHA32F 1
int vr_set_framebuffer_format(vr_handle h, int format);
int vr_local_rows(vr_handle h);
/* launch on a caller-owned HIP stream (hipStream_t as void*); NULL = own stream */
int vr_set_stream(vr_handle h, void *hip_stream);
/* render into a caller-owned device buffer of fb_w*fb_h*4 floats; NULL = own target */
int vr_set_framebuffer_external(vr_handle h, void *device_rgba);

/* ---- render(): src/RendererCore.cpp:138-163 (RendererGUI.cpp:101) ----------- */
/* Launches the ray-march kernel into the off-screen target, times it with HIP
   events and adds the ms to kerneltime_sum (blocking, like the reference's
   GL_TIME_ELAPSED read-back). */
int vr_render(vr_handle h);
/* same launch without events or host synchronisation (for benches / graphs) */
int vr_render_async(vr_handle h);
int vr_synchronize(vr_handle h);
/* kerneltime_sum read-and-zero (RendererGUI.cpp:58,60) */
float vr_kernel_ms_take(vr_handle h);
/* instrumented (untimed) launch: number of volume fetches per pixel / total */
int vr_count_samples(vr_handle h, uint64_t *total, uint32_t *per_pixel, size_t n_pixels);
void *vr_framebuffer_device(vr_handle h);
int vr_read_pixels(vr_handle h, float *rgba, size_t n_floats);     /* D2H of the target */
/* the same frame as RGBA8 (fb_w*fb_h*4 bytes, row 0 = bottom like the target), converted on the
   device with glReadPixels' rule round(clamp(c,0,1)*255) (the precision of the reference's own
   read-back, src/RendererCore.cpp:170): a quarter of the bytes over PCIe for display */
int vr_read_pixels_rgba8(vr_handle h, unsigned char *rgba8, size_t n_bytes);
/* presentation for a display that is not this GPU (replaces the reference's on-GPU blit of the target to the back
   buffer, src/RendererCore.cpp:158-162): call once per frame after vr_render.  The frame is converted to RGBA8 on the
   launch stream and copied into one of THREE pinned host buffers on a separate copy stream, so the copy of frame i runs
   under the kernel of frame i + 1; *frame receives the PREVIOUS call's frame (fb_w x fb_h RGBA8, row 0 = bottom; on the
   first call: this frame, after a wait).  The pointer stays valid until the next-but-one call (call n hands out
   slot (n - 1) % 3, call n + 1 fills slot (n + 1) % 3, call n + 2 overwrites it).  One frame of display
   latency for an interactive loop that never waits on PCIe: 0.46 ms kernel + 8 MB copy overlapped, instead of 1.3 ms
   for kernel + blocking RGBA32F read-back. */
int vr_present_rgba8(vr_handle h, const unsigned char **frame);
/* saveImage(fn, ext) (src/RendererCore.cpp:165-182): ext ".png" | ".jpg" (quality 100, as
   :177) | ".bmp" of the reference's dialog (RendererGUI.cpp:221), plus ".ppm" */
int vr_save_image(vr_handle h, const char *path, const char *ext);
/* the writers behind vr_save_image for an RGB8 image already in host memory (rows top first,
   stride in bytes); host only, no handle.  Returns VR_OK or VR_E_IO / VR_E_INVALID. */
int vr_write_image_rgb8(const char *path, const char *ext, int width, int height,
                        const unsigned char *rgb, int stride_bytes);

/* ---- one node, several GPUs, one process (shards the single dispatch of
        src/RendererCore.cpp:149-151 so that a caller shaped like RendererGUI::run,
        src/RendererGUI.cpp:100-101, uses every GPU by calling vr_group_render where it called
        render()).  One renderer per device: the volume is replicated (load / generate it on every
        member), the image rows are sharded, the shards are gathered on devices[0] -- over RCCL
        (grouped ncclSend/ncclRecv across xGMI, librccl loaded on first use) when the devices are
        distinct, with peer copies otherwise -- and assembled there into one RGBA32F frame.
        Members are ordinary handles: configure them with the calls above (the same values on every
        member); their row range / stripes / target are owned by the group. ------------------------ */
typedef struct vr_group *vr_group_handle;
int vr_group_create(vr_group_handle *out, const int *devices, int n);
void vr_group_destroy(vr_group_handle g);
int vr_group_size(vr_group_handle g);
vr_handle vr_group_member(vr_group_handle g, int rank);
/* vr_setup on every member + the shard plan: partition 0 = cyclic stripes of `stripe_rows` rows
   (balanced: only ~75 % of the rows hit the box at the default camera), 1 = contiguous row blocks */
int vr_group_setup(vr_group_handle g, int win_w, int win_h, int fb_w, int fb_h, int partition, int stripe_rows);
/* 1 (default): RCCL when every member has its own device; 0: always peer copies; 2: like 1, and a
   one-member group also creates its communicator and every shard -- the root's own included --
   travels through a grouped ncclSend/ncclRecv (on a one-GPU box: a send to self, which executes
   the same RCCL calls, datatype, counts and stream wiring as the multi-GPU gather).
   Call before vr_group_setup. */
int vr_group_set_transport(vr_group_handle g, int use_rccl);
const char *vr_group_transport(vr_group_handle g);     /* what vr_group_setup chose */
/* render(): every member's shard kernel (concurrently, one stream per device), the gather and the
   assembly; blocks until the frame is complete on devices[0].  Adds the slowest member's kernel
   time to the group's kerneltime_sum.  == vr_group_render_async + vr_group_wait. */
int vr_group_render(vr_group_handle g);
/* the same frame without the block (replaces the reference's blocking timer read-back,
   src/RendererCore.cpp:152, for callers that can run a frame ahead): vr_group_render_async
   enqueues the next frame into one of THREE frame slots -- shard kernels on the members' render
   streams, gather and assembly on separate transfer streams -- and returns; at most two frames
   may be in flight (VR_E_INVALID otherwise), so the slot of the last completed frame is never the
   one a frame issued next is assembled into: what vr_group_framebuffer_device returned stays
   that frame until the next vr_group_wait.  vr_group_wait blocks until the OLDEST frame in
   flight is assembled and makes it the frame vr_group_framebuffer_device / vr_group_read_pixels
   return.  Keeping one frame in flight overlaps the gather of frame i with the kernels of
   frame i + 1. */
int vr_group_render_async(vr_group_handle g);
int vr_group_wait(vr_group_handle g);
float vr_group_kernel_ms_take(vr_group_handle g);
void *vr_group_framebuffer_device(vr_group_handle g);   /* fb_w x fb_h RGBA32F on devices[0] */
int vr_group_read_pixels(vr_group_handle g, float *rgba, size_t n_floats);
int vr_group_present_rgba8(vr_group_handle g, const unsigned char **frame);   /* vr_present_rgba8 of the assembled frame */
const char *vr_group_last_error(vr_group_handle g);

/* name of the kernel variant the last vr_render* launched (for profiles/tests) */
const char *vr_last_kernel_name(vr_handle h);

#ifdef __cplusplus
}
#endif
#endif /* VR_CORE_H */
