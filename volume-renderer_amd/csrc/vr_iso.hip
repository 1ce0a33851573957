// vr_iso.hip -- the first-hit isosurface kernel (vr_set_isosurface): the composite mode's ray and sample positions, the first
// sample at or above the iso value, a linear refinement between it and the sample before, a central-difference normal and a
// two-sided headlight.  The definition, step by step, is in include/vr_core.h and DESIGN.md section 1; tests/iso_ref/iso_ref.c
// restates it on the CPU and tests/test_isosurface_gpu.py holds this kernel to it bit for bit.
//
// Its own translation units (VR_ISO_TU = 0: 8-bit volumes and the entry point, 1: 16-bit volumes; the build always sets it, and
// VR_CODE_UNIT registers each for the pre-load), like vr_tslab.hip; launched through mode_dispatch.h: the vr_kernels.hip units,
// FrameParams and LaunchConfig are untouched by the mode, the iso value, the depth target and the skip grid are extra
// kernel arguments.  Arithmetic contract as in vr_kernels.hip: one correctly rounded fp32 operation per step, nothing
// contracted (-ffp-contract=off), the only fused operations are explicit: TRILINEAR's lerps (tri_lerp) and the certified
// texcoord division (div_cert).
//
// Shape: the generic kernel's -- one pixel per lane, 8x8 pixels per wavefront, 16x16-pixel tiles of four wavefronts dealt to
// the XCDs by tile_of_block().  Empty-space skipping per 8^3 cell: a sample's taps lie within one voxel of its NEAREST voxel
// (TRILINEAR: of the lower tap), so a sample in a cell whose DILATED maximum (the cell and its 26 neighbours) is below the iso
// value is below it too and is not fetched.  The grid is read when the ray enters a new cell, not per step; positions still
// advance sample by sample with the shader's additions, so hits, counts and frames are the same bits with and without it.
// The ray start and the skip cell are vr_march.h's, shared with vr_shade.hip; gradient, normal and headlight are written out here.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mode_dispatch.h"
#include "vr_code_unit.h"
#include "vr_march.h"
#include "vr_iso.h"

#ifndef VR_ISO_TU
#error "VR_ISO_TU: the unit number comes from the build"
#endif

namespace vr {

template <typename VoxelT, int LAYOUT, int FILTER, bool SKIP, bool BIG>
__global__ __launch_bounds__(256) void raymarch_iso_kernel(const FrameParams P, const int divmode, const uint32_t vol_bytes,
                                                           const VoxelT *__restrict__ vol, const float4 *__restrict__ tf,
                                                           float4 *__restrict__ fb, uint32_t *__restrict__ spp,
                                                           float *__restrict__ depth, const uint16_t *__restrict__ grid,
                                                           const float iso_s, const unsigned tiles_x, const unsigned tiles_y)
{
    unsigned tx, ty;
    tile_of_block(blockIdx.x, tiles_x, tiles_y, tx, ty);
    if (tx == 0xffffffffu) return;
    int lx, ly, px, py;
    if (!tile_pixel(P, tx, ty, lx, ly, px, py)) return;

    const Ray ray = compute_ray(P, (float)px + 0.5f, (float)py + 0.5f);
    float t_min = 0.0f, t_max = 0.0f;
    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, c3 = 0.0f, t_hit = __builtin_inff();
    uint32_t samples = 0;
    if (intersect_ray_aabb(P, ray, t_min, t_max)) {
        const VolumeSampler<VoxelT, LAYOUT, BIG> S(P, vol, vol_bytes);
        auto sample_at = [&](float tcx, float tcy, float tcz) -> float {
            if (FILTER == 0)
                return S.voxel(nearest_index(tcx, P.fdim[0], P.nx), nearest_index(tcy, P.fdim[1], P.ny), nearest_index(tcz, P.fdim[2], P.nz));
            return S.trilinear(tcx * P.fdim[0] - 0.5f, tcy * P.fdim[1] - 0.5f, tcz * P.fdim[2] - 0.5f);
        };

        const RayStart R = ray_start(P, ray, t_min);
        const float p0x = R.p0x, p0y = R.p0y, p0z = R.p0z, dsx = R.dsx, dsy = R.dsy, dsz = R.dsz;
        float qx = p0x, qy = p0y, qz = p0z;          // q_i
        float rx = p0x, ry = p0y, rz = p0z;          // q_{i-1}
        float s_prev = 0.0f, s_hit = 0.0f;
        bool prev_fetched = false, hit = false;
        int i = 0;
        SkipCell skip;
        // ---- the march: the composite mode's positions and box-exit test (without its dest.a term), no window, no compositing
        for (; i < P.max_steps; i++) {
            if (P.accum == 1) {
                const float fi = (float)i;
                qx = p0x + fi * dsx; qy = p0y + fi * dsy; qz = p0z + fi * dsz;
            }
            float tcx, tcy, tcz;
            texcoord(P, divmode, qx, qy, qz, tcx, tcy, tcz);
            if (tcx > 1.0f || tcy > 1.0f || tcz > 1.0f || tcx < 0.0f || tcy < 0.0f || tcz < 0.0f) break;
            bool fetch = true;
            if (SKIP) {
                // the sample's cell: its NEAREST voxel (TRILINEAR: its lower tap), >> 3
                int ci, cj, ck;
                if (FILTER == 0) {
                    ci = nearest_index(tcx, P.fdim[0], P.nx); cj = nearest_index(tcy, P.fdim[1], P.ny); ck = nearest_index(tcz, P.fdim[2], P.nz);
                } else {
                    ci = lower_tap(tcx * P.fdim[0] - 0.5f, P.nx);
                    cj = lower_tap(tcy * P.fdim[1] - 0.5f, P.ny);
                    ck = lower_tap(tcz * P.fdim[2] - 0.5f, P.nz);
                }
                fetch = !skip.enter(P, grid, ci, cj, ck, [&](uint16_t cell_max) { return (float)cell_max < iso_s; });
            }
            if (fetch) {
                const float s = sample_at(tcx, tcy, tcz);
                if (s >= iso_s) { s_hit = s; hit = true; break; }
                s_prev = s;
            }
            prev_fetched = fetch;
            rx = qx; ry = qy; rz = qz;
            if (P.accum == 0) { qx += dsx; qy += dsy; qz += dsz; }
        }
        samples = (uint32_t)(hit ? i + 1 : i);
        if (hit) {
            // ---- refinement: h = q_{i-1} + f * (q_i - q_{i-1}),  f = (iso - s_{i-1}) / (s_i - s_{i-1});  h = q_0 at i = 0
            float hx = qx, hy = qy, hz = qz;
            if (i > 0) {
                if (!prev_fetched) {          // the step before was skipped: fetch s_{i-1} now
                    float tcx, tcy, tcz;
                    texcoord(P, divmode, rx, ry, rz, tcx, tcy, tcz);
                    s_prev = sample_at(tcx, tcy, tcz);
                }
                const float f = (iso_s - s_prev) / (s_hit - s_prev);
                hx = rx + f * (qx - rx); hy = ry + f * (qy - ry); hz = rz + f * (qz - rz);
            }
            // ---- gradient: central differences of the same sampler at h, +-1 voxel per volume axis, clamped to the edge
            float tcx, tcy, tcz;
            texcoord(P, divmode, hx, hy, hz, tcx, tcy, tcz);
            float gx, gy, gz;
            if (FILTER == 0) {
                const int vi = nearest_index(tcx, P.fdim[0], P.nx), vj = nearest_index(tcy, P.fdim[1], P.ny), vk = nearest_index(tcz, P.fdim[2], P.nz);
                gx = S.voxel(clampi(vi + 1, 0, P.nx - 1), vj, vk) - S.voxel(clampi(vi - 1, 0, P.nx - 1), vj, vk);
                gy = S.voxel(vi, clampi(vj + 1, 0, P.ny - 1), vk) - S.voxel(vi, clampi(vj - 1, 0, P.ny - 1), vk);
                gz = S.voxel(vi, vj, clampi(vk + 1, 0, P.nz - 1)) - S.voxel(vi, vj, clampi(vk - 1, 0, P.nz - 1));
            } else {
                const float u = tcx * P.fdim[0] - 0.5f, v = tcy * P.fdim[1] - 0.5f, w = tcz * P.fdim[2] - 0.5f;
                gx = S.trilinear(u + 1.0f, v, w) - S.trilinear(u - 1.0f, v, w);
                gy = S.trilinear(u, v + 1.0f, w) - S.trilinear(u, v - 1.0f, w);
                gz = S.trilinear(u, v, w + 1.0f) - S.trilinear(u, v, w - 1.0f);
            }
            // volume axes -> box axes: the view's permutation, the z flip, dim / ext per axis (anisotropic spacing)
            const float Gx = gx * (P.fdim[0] / P.ext[0]);
            float Gy, Gz;
            if (P.view_top == 1) { Gy = gz * (P.fdim[2] / P.ext[1]); Gz = gy * (P.fdim[1] / P.ext[2]); }
            else if (P.view_bottom == 1) { Gy = -(gz * (P.fdim[2] / P.ext[1])); Gz = -(gy * (P.fdim[1] / P.ext[2])); }
            else { Gy = gy * (P.fdim[1] / P.ext[1]); Gz = -(gz * (P.fdim[2] / P.ext[2])); }
            // N = normalize(-G) = v * (1 / sqrt(dot)), dot summed from the last component to the first; G = 0: N = -dir
            float nx = -Gx, ny = -Gy, nz = -Gz;
            const float dot = (nz * nz + ny * ny) + nx * nx;
            if (dot == 0.0f) {
                nx = -ray.dx; ny = -ray.dy; nz = -ray.dz;
            } else {
                const float rn = 1.0f / sqrtf(dot);
                nx = nx * rn; ny = ny * rn; nz = nz * rn;
            }
            // two-sided headlight, L = V = H = -dir
            float d = (nz * -ray.dz + ny * -ray.dy) + nx * -ray.dx;
            if (d < 0.0f) d = -d;
            const float d2 = d * d, d4 = d2 * d2, d8 = d4 * d4, spec = d8 * d8;
            const float lit = 0.15f + 0.65f * d, hl = 0.2f * spec;
            // base colour: the transfer function's rgb at the windowed iso value (the generic kernel's index rule), else white
            float b0 = 1.0f, b1 = 1.0f, b2 = 1.0f;
            if (P.tf_len > 1) {
                const float s = window_map(P, iso_s, DIV_EXACT);
                const int idx = tf_index(P, s);
                const float4 t = tf[idx];
                b0 = t.x; b1 = t.y; b2 = t.z;
            }
            c0 = gl_min(b0 * lit + hl, 1.0f);
            c1 = gl_min(b1 * lit + hl, 1.0f);
            c2 = gl_min(b2 * lit + hl, 1.0f);
            c3 = 1.0f;
            // depth: t = (h - o) . dir, summed from the last component to the first
            t_hit = ((hz - ray.oz) * ray.dz + (hy - ray.oy) * ray.dy) + (hx - ray.ox) * ray.dx;
        }
    }
    const size_t pix = (size_t)(P.fb_compact ? ly : py) * (size_t)P.img_w + (size_t)px;
    fb[pix] = make_float4(c0, c1, c2, c3);
    depth[pix] = t_hit;
    if (spp) spp[pix] = samples;
}

template <typename VoxelT>
static hipError_t launch_iso_type(const FrameParams &P, const LaunchConfig &L, const IsoArgs &A, const void *vol, const float4 *tf,
                                  float4 *fb, uint32_t *spp, hipStream_t st)
{
    const Tiles16 t = launch_tiles16(P);
    const int div = texcoord_divmode(L);
    const dim3 grid(padded_blocks(t.x, t.y)), block(256);
    return dispatch_mode(L, BoolAxis{A.skip_grid != nullptr}, [&](auto LAY, auto FIL, auto SKIP, auto BIG) {
        hipLaunchKernelGGL((raymarch_iso_kernel<VoxelT, LAY(), FIL(), SKIP(), BIG()>), grid, block, 0, st, P, div,
                           BIG() ? 0u : (uint32_t)L.vol_bytes32, (const VoxelT *)vol, tf, fb, spp, A.depth, A.skip_grid, A.iso_s, t.x, t.y);
        return hipGetLastError();
    });
}

VR_CODE_UNIT(iso, VR_ISO_TU, "isosurface", WARM_LOAD_SHADER)

#define VR_ISO_ARGS const FrameParams &P, const LaunchConfig &L, const IsoArgs &A, const void *vol, const float4 *tf, float4 *fb, uint32_t *spp, hipStream_t st
#if VR_ISO_TU == 1
hipError_t launch_iso_u16(VR_ISO_ARGS) { return launch_iso_type<uint16_t>(P, L, A, vol, tf, fb, spp, st); }
#else
// the unit of 8-bit volumes also carries the entry point
hipError_t launch_iso_u16(VR_ISO_ARGS);

hipError_t launch_raymarch_iso(VR_ISO_ARGS, const char **kernel_name)
{
    if (kernel_name) *kernel_name = "raymarch_iso_kernel";
    if (launch_local_rows(P) <= 0 || P.img_w <= 0) return hipSuccess;
    if (!A.depth) return hipErrorInvalidValue;
    return L.bytes_per_voxel == 1 ? launch_iso_type<uint8_t>(P, L, A, vol, tf, fb, spp, st) : launch_iso_u16(P, L, A, vol, tf, fb, spp, st);
}
#endif
#undef VR_ISO_ARGS

}  // namespace vr
