// vr_shade.hip -- the gradient-lit composite kernel (vr_set_shading): the composite mode's march, window, classification and
// compositing, with each visible sample's colour lit by a central-difference normal and the isosurface mode's two-sided
// headlight.  The definition, step by step, is in include/vr_core.h and DESIGN.md section 1.3; tests/shade_ref/shade_ref.c
// restates it on the CPU and tests/test_shading_gpu.py holds this kernel to it bit for bit.
//
// Its own translation units (VR_SHADE_TU = 0: 8-bit volumes and the entry point, 1: 16-bit volumes; the build always sets it, and
// VR_CODE_UNIT registers each for the pre-load), like vr_iso.hip; launched through mode_dispatch.h: the vr_kernels.hip units,
// FrameParams and LaunchConfig are untouched by the mode; the coefficients and the skip grid are extra kernel arguments.
// Arithmetic contract as in vr_kernels.hip: one correctly rounded fp32 operation per step, nothing contracted
// (-ffp-contract=off), the only fused operations are explicit: TRILINEAR's lerps (tri_lerp) and the certified divisions
// (div_cert: texture coordinates and the window).
//
// Shape: the isosurface kernel's -- one pixel per lane, 8x8 pixels per wavefront, 16x16-pixel tiles of four wavefronts dealt to
// the XCDs by tile_of_block().  The 256-entry transfer function is staged in LDS (4 KiB): every sample reads one entry.
// Samples with alpha 0 take no gradient (their contribution is finite rgb x 0 either way).  NEAREST gradients are six voxel
// loads around the sample's voxel; TRILINEAR gradients are six sampler evaluations, each with its own floor and taps: in fp32
// floor(u + 1) is not always floor(u) + 1, so taps are not shared between them.
// Empty-space skipping per 8^3 cell: a sample's taps lie within one voxel of its NEAREST voxel (TRILINEAR: of its lower tap),
// so a sample in a cell whose DILATED maximum is <= the threshold (RendererCore::zeroAlphaThreshold) classifies to alpha 0 and
// is not fetched: it would add +-0 to dest, which is never -0.  Positions still advance sample by sample and every step is
// counted, so frames and counts are the same bits with and without it.
// The ray start and the skip cell are vr_march.h's, shared with vr_iso.hip; gradient, normal and headlight are written out here.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mode_dispatch.h"
#include "vr_code_unit.h"
#include "vr_march.h"
#include "vr_shade.h"

#ifndef VR_SHADE_TU
#error "VR_SHADE_TU: the unit number comes from the build"
#endif

namespace vr {

template <typename VoxelT, int LAYOUT, int FILTER, bool SKIP, bool BIG>
__global__ __launch_bounds__(256) void raymarch_shade_kernel(const FrameParams P, const int divmode, const int divmode_win,
                                                             const uint32_t vol_bytes, const VoxelT *__restrict__ vol,
                                                             const float4 *__restrict__ tf, float4 *__restrict__ fb,
                                                             uint32_t *__restrict__ spp, const uint16_t *__restrict__ grid,
                                                             const int32_t skip_thresh, const float k_amb, const float k_dif,
                                                             const float k_spec, const int spec_squarings, const unsigned tiles_x,
                                                             const unsigned tiles_y)
{
    __shared__ float4 s_tf[256];
    unsigned tx, ty;
    tile_of_block(blockIdx.x, tiles_x, tiles_y, tx, ty);
    if (tx == 0xffffffffu) return;                 // (a padding block: all of its threads)
    const bool use_tf = P.tf_len > 1;              // (the launcher refuses tf_len > 256)
    if (use_tf && (int)threadIdx.x < P.tf_len) s_tf[threadIdx.x] = tf[threadIdx.x];
    __syncthreads();
    int lx, ly, px, py;
    if (!tile_pixel(P, tx, ty, lx, ly, px, py)) return;

    const Ray ray = compute_ray(P, (float)px + 0.5f, (float)py + 0.5f);
    float t_min = 0.0f, t_max = 0.0f;
    float d0 = 0.0f, d1 = 0.0f, d2 = 0.0f, d3 = 0.0f;
    uint32_t fetches = 0;
    if (intersect_ray_aabb(P, ray, t_min, t_max)) {
        const VolumeSampler<VoxelT, LAYOUT, BIG> S(P, vol, vol_bytes);
        const RayStart R = ray_start(P, ray, t_min);
        const float p0x = R.p0x, p0y = R.p0y, p0z = R.p0z, dsx = R.dsx, dsy = R.dsy, dsz = R.dsz;
        // the headlight L = V = H = -dir, and the box-space scale of each volume axis (dim / ext, the view's permutation)
        const float lx_ = -ray.dx, ly_ = -ray.dy, lz_ = -ray.dz;
        const float gsx = P.fdim[0] / P.ext[0];
        const float gsy = (P.view_top == 1 || P.view_bottom == 1) ? P.fdim[2] / P.ext[1] : P.fdim[1] / P.ext[1];
        const float gsz = (P.view_top == 1 || P.view_bottom == 1) ? P.fdim[1] / P.ext[2] : P.fdim[2] / P.ext[2];
        float qx = p0x, qy = p0y, qz = p0z;
        SkipCell skip;
        for (int i = 0; i < P.max_steps; i++) {
            if (P.accum == 1) {
                const float fi = (float)i;
                qx = p0x + fi * dsx; qy = p0y + fi * dsy; qz = p0z + fi * dsz;
            }
            // cartesianToTextureCoord (VolumeRenderer.cs:175-192), as the generic kernel computes it
            float ux = qx + P.half[0], uy = qy + P.half[1], uz = qz + P.half[2];
            if (divmode == DIV_CERT) {
                ux = div_cert(ux, P.ext[0], P.rext[0]);
                uy = div_cert(uy, P.ext[1], P.rext[1]);
                uz = div_cert(uz, P.ext[2], P.rext[2]);
            } else {
                ux = ux / P.ext[0]; uy = uy / P.ext[1]; uz = uz / P.ext[2];
            }
            const float uzr = uz;
            uz = 1.0f - uz;
            float tcx, tcy, tcz;
            if (P.view_top == 1) { tcx = ux; tcy = uzr; tcz = uy; }
            else if (P.view_bottom == 1) { tcx = ux; tcy = uz; tcz = 1.0f - uy; }
            else { tcx = ux; tcy = uy; tcz = uz; }
            if (tcx > 1.0f || tcy > 1.0f || tcz > 1.0f || tcx < 0.0f || tcy < 0.0f || tcz < 0.0f || d3 >= 0.95f) break;
            fetches++;
            // the sample's voxel (NEAREST) or its lower tap and continuous coordinates (TRILINEAR)
            int vi, vj, vk;
            float u = 0.0f, v = 0.0f, w = 0.0f;
            if (FILTER == 0) {
                vi = nearest_index(tcx, P.fdim[0], P.nx); vj = nearest_index(tcy, P.fdim[1], P.ny); vk = nearest_index(tcz, P.fdim[2], P.nz);
            } else {
                u = tcx * P.fdim[0] - 0.5f; v = tcy * P.fdim[1] - 0.5f; w = tcz * P.fdim[2] - 0.5f;
                vi = lower_tap(u, P.nx); vj = lower_tap(v, P.ny); vk = lower_tap(w, P.nz);
            }
            bool visible = true;
            if (SKIP) {
                visible = !skip.enter(P, grid, vi, vj, vk, [&](uint16_t cell_max) { return (int32_t)cell_max <= skip_thresh; });
            }
            if (visible) {
                float s = FILTER == 0 ? S.voxel(vi, vj, vk) : S.trilinear(u, v, w);
                // window (VolumeRenderer.cs:122-124; Q4: max == min defined as 0), the division certified like the composite kernels'
                s = window_map(P, s, divmode_win);
                float c0 = s, c1 = s, c2 = s, a = s;
                if (use_tf) {
                    const int idx = tf_index(P, s);
                    const float4 t = s_tf[idx];
                    c0 = t.x; c1 = t.y; c2 = t.z; a = t.w;
                }
                a *= P.alpha_scale;
                if (a != 0.0f) {
                    // ---- gradient: central differences of the same sampler at the sample, +-1 voxel per volume axis, clamped
                    float gx, gy, gz;
                    if (FILTER == 0) {
                        gx = S.voxel(clampi(vi + 1, 0, P.nx - 1), vj, vk) - S.voxel(clampi(vi - 1, 0, P.nx - 1), vj, vk);
                        gy = S.voxel(vi, clampi(vj + 1, 0, P.ny - 1), vk) - S.voxel(vi, clampi(vj - 1, 0, P.ny - 1), vk);
                        gz = S.voxel(vi, vj, clampi(vk + 1, 0, P.nz - 1)) - S.voxel(vi, vj, clampi(vk - 1, 0, P.nz - 1));
                    } else {
                        gx = S.trilinear(u + 1.0f, v, w) - S.trilinear(u - 1.0f, v, w);
                        gy = S.trilinear(u, v + 1.0f, w) - S.trilinear(u, v - 1.0f, w);
                        gz = S.trilinear(u, v, w + 1.0f) - S.trilinear(u, v, w - 1.0f);
                    }
                    // volume axes -> box axes: the view's permutation, the z flip, dim / ext per axis
                    const float Gx = gx * gsx;
                    float Gy, Gz;
                    if (P.view_top == 1) { Gy = gz * gsy; Gz = gy * gsz; }
                    else if (P.view_bottom == 1) { Gy = -(gz * gsy); Gz = -(gy * gsz); }
                    else { Gy = gy * gsy; Gz = -(gz * gsz); }
                    // N = normalize(-G) = v * (1 / sqrt(dot)), dot summed from the last component to the first; G = 0: N = -dir
                    float nx = -Gx, ny = -Gy, nz = -Gz;
                    const float dot = (nz * nz + ny * ny) + nx * nx;
                    if (dot == 0.0f) {
                        nx = lx_; ny = ly_; nz = lz_;
                    } else {
                        const float rn = 1.0f / sqrtf(dot);
                        nx = nx * rn; ny = ny * rn; nz = nz * rn;
                    }
                    // ---- two-sided headlight
                    float d = (nz * lz_ + ny * ly_) + nx * lx_;
                    if (d < 0.0f) d = -d;
                    float spec = d;
                    for (int k = 0; k < spec_squarings; k++) spec = spec * spec;
                    const float lit = k_amb + k_dif * d, hl = k_spec * spec;
                    c0 = gl_min(c0 * lit + hl, 1.0f);
                    c1 = gl_min(c1 * lit + hl, 1.0f);
                    c2 = gl_min(c2 * lit + hl, 1.0f);
                }
                // ---- compositing (VolumeRenderer.cs:130-135)
                c0 *= a; c1 *= a; c2 *= a;
                const float om = 1.0f - d3;
                d0 += c0 * om; d1 += c1 * om; d2 += c2 * om; d3 += a * om;
                if (d3 > 0.99f) break;
            }
            if (P.accum == 0) { qx += dsx; qy += dsy; qz += dsz; }
        }
    }
    const size_t pix = (size_t)(P.fb_compact ? ly : py) * (size_t)P.img_w + (size_t)px;
    store_pixel(P, fb, pix, d0, d1, d2, d3);
    if (spp) spp[pix] = fetches;
}

template <typename VoxelT>
static hipError_t launch_shade_type(const FrameParams &P, const LaunchConfig &L, const ShadeArgs &A, const void *vol, const float4 *tf,
                                    float4 *fb, uint32_t *spp, hipStream_t st)
{
    const Tiles16 t = launch_tiles16(P);
    const int div = texcoord_divmode(L), div_win = window_divmode(L);
    const dim3 grid(padded_blocks(t.x, t.y)), block(256);
    return dispatch_mode(L, BoolAxis{A.skip_grid != nullptr}, [&](auto LAY, auto FIL, auto SKIP, auto BIG) {
        hipLaunchKernelGGL((raymarch_shade_kernel<VoxelT, LAY(), FIL(), SKIP(), BIG()>), grid, block, 0, st, P, div, div_win,
                           BIG() ? 0u : (uint32_t)L.vol_bytes32, (const VoxelT *)vol, tf, fb, spp, A.skip_grid, A.skip_thresh, A.ambient,
                           A.diffuse, A.specular, A.spec_squarings, t.x, t.y);
        return hipGetLastError();
    });
}

VR_CODE_UNIT(shade, VR_SHADE_TU, "shading", WARM_LOAD_SHADER)

#define VR_SHADE_ARGS const FrameParams &P, const LaunchConfig &L, const ShadeArgs &A, const void *vol, const float4 *tf, float4 *fb, uint32_t *spp, hipStream_t st
#if VR_SHADE_TU == 1
hipError_t launch_shade_u16(VR_SHADE_ARGS) { return launch_shade_type<uint16_t>(P, L, A, vol, tf, fb, spp, st); }
#else
// the unit of 8-bit volumes also carries the entry point
hipError_t launch_shade_u16(VR_SHADE_ARGS);

hipError_t launch_raymarch_shade(VR_SHADE_ARGS, const char **kernel_name)
{
    if (kernel_name) *kernel_name = "raymarch_shade_kernel";
    if (launch_local_rows(P) <= 0 || P.img_w <= 0) return hipSuccess;
    if (P.tf_len > 256 || (P.tf_len > 1 && !tf) || A.spec_squarings < 0 || A.spec_squarings > 7) return hipErrorInvalidValue;
    return L.bytes_per_voxel == 1 ? launch_shade_type<uint8_t>(P, L, A, vol, tf, fb, spp, st) : launch_shade_u16(P, L, A, vol, tf, fb, spp, st);
}
#endif
#undef VR_SHADE_ARGS

}  // namespace vr
