// vr_iso.hip -- the first-hit isosurface kernel (vr_set_isosurface): the composite mode's ray and sample positions, the first
// sample at or above the iso value, a linear refinement between it and the sample before, a central-difference normal and a
// two-sided headlight.  The definition, step by step, is in include/vr_core.h and DESIGN.md section 1; tests/iso_ref/iso_ref.c
// restates it on the CPU and tests/test_isosurface_gpu.py holds this kernel to it bit for bit.
//
// Its own translation units (VR_ISO_TU = 0: 8-bit volumes, 1: 16-bit volumes), like vr_tslab.hip: the vr_kernels.hip units,
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
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vr_device.h"
#include "vr_iso.h"

#ifndef VR_ISO_TU
#define VR_ISO_TU -1
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
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const int lx = (int)(tx * 16u + (wave & 1u) * 8u + (lane & 7u));
    const int ly = (int)(ty * 16u + (wave >> 1) * 8u + (lane >> 3));
    int px = lx, py;
    if (P.stripe_count > 1) {
        const int s = ly / P.stripe_rows, r = ly % P.stripe_rows;
        py = (s * P.stripe_count + P.stripe_index) * P.stripe_rows + r;
    } else {
        py = P.row_begin + ly;
    }
    if (px >= P.col_lim || py >= P.row_lim || py >= P.row_end) return;

    const Ray ray = compute_ray(P, (float)px + 0.5f, (float)py + 0.5f);
    float t_min = 0.0f, t_max = 0.0f;
    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, c3 = 0.0f, t_hit = __builtin_inff();
    uint32_t samples = 0;
    if (intersect_ray_aabb(P, ray, t_min, t_max)) {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)vol, 0, BIG ? 0 : (int)pair_load_extent(vol_bytes), 0x00020000);
        // per-axis terms of VoxelAddr<LAYOUT, false>::at(i, j, k) = X(i) + Y(j) + Z(k)  (mod 2^32), as in the generic kernel
        auto term_x = [&](int i) -> uint32_t {
            return LAYOUT == 0 ? (uint32_t)i : mad_u24((uint32_t)i >> BRICK_LX, 64u - (uint32_t)BRICK_X, (uint32_t)i);
        };
        auto term_y = [&](int j) -> uint32_t {
            if (LAYOUT == 0) return mad_u24((uint32_t)j, (uint32_t)P.nx, 0u);
            return mad_u24(BRICK_LY ? (uint32_t)j >> BRICK_LY : (uint32_t)j, P.bstride_y, BRICK_LY ? (uint32_t)j << BRICK_LX : 0u);
        };
        auto term_z = [&](int k) -> uint32_t {
            if (LAYOUT == 0) return mad_u24(mad_u24((uint32_t)k, (uint32_t)P.ny, 0u), (uint32_t)P.nx, 0u);
            return mad_u24(BRICK_LZ ? (uint32_t)k >> BRICK_LZ : (uint32_t)k, P.bstride_z, BRICK_LZ ? (uint32_t)k << (BRICK_LX + BRICK_LY) : 0u);
        };
        auto tap = [&](uint32_t off) -> float { return (float)VoxelFetch<VoxelT, false>::load(vol, rs, off); };
        // NEAREST: voxel (i, j, k), indices already clamped
        auto voxel = [&](int i, int j, int k) -> float {
            return BIG ? fetch_voxel<VoxelT, LAYOUT>(P, vol, i, j, k) : tap(term_x(i) + term_y(j) + term_z(k));
        };
        // TRILINEAR at the sampler's own continuous coordinates (u, v, w) = tc * dim - 0.5: GL's linear rule, taps clamped to
        // the edge, x then y then z, each lerp one fma.  32-bit offsets fetch each x pair with one load (the generic kernel's pair loads)
        auto trilinear = [&](float u, float v, float w) -> float {
            const float fu = floorf(u), fv = floorf(v), fw = floorf(w);
            const float ax = u - fu, ay = v - fv, az = w - fw;
            const int iu = (int)fu, iv = (int)fv, iw = (int)fw;
            const int i0 = clampi(iu, 0, P.nx - 1), i1 = clampi(iu + 1, 0, P.nx - 1);
            const int j0 = clampi(iv, 0, P.ny - 1), j1 = clampi(iv + 1, 0, P.ny - 1);
            const int k0 = clampi(iw, 0, P.nz - 1), k1 = clampi(iw + 1, 0, P.nz - 1);
            float c000, c100, c010, c110, c001, c101, c011, c111;
            if (BIG) {
                c000 = fetch_voxel<VoxelT, LAYOUT>(P, vol, i0, j0, k0); c100 = fetch_voxel<VoxelT, LAYOUT>(P, vol, i1, j0, k0);
                c010 = fetch_voxel<VoxelT, LAYOUT>(P, vol, i0, j1, k0); c110 = fetch_voxel<VoxelT, LAYOUT>(P, vol, i1, j1, k0);
                c001 = fetch_voxel<VoxelT, LAYOUT>(P, vol, i0, j0, k1); c101 = fetch_voxel<VoxelT, LAYOUT>(P, vol, i1, j0, k1);
                c011 = fetch_voxel<VoxelT, LAYOUT>(P, vol, i0, j1, k1); c111 = fetch_voxel<VoxelT, LAYOUT>(P, vol, i1, j1, k1);
            } else {
                const uint32_t x0 = term_x(i0), x1 = term_x(i1), y0 = term_y(j0), y1 = term_y(j1);
                const uint32_t z0 = term_z(k0), z1 = term_z(k1);
                const bool pair = i1 == i0 + 1 && (LAYOUT == 0 || ((uint32_t)i0 & (BRICK_X - 1u)) != BRICK_X - 1u);
                auto tap2 = [&](uint32_t off, float &lo, float &hi) {
                    if (sizeof(VoxelT) == 1) {
                        const uint32_t q = (uint32_t)(uint16_t)__builtin_amdgcn_raw_buffer_load_b16(rs, (int)off, 0, 0);
                        lo = (float)(q & 0xffu); hi = (float)(q >> 8);
                    } else {
                        const uint32_t q = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs, (int)(off << 1), 0, 0);
                        lo = (float)(q & 0xffffu); hi = (float)(q >> 16);
                    }
                };
                tap2(x0 + y0 + z0, c000, c100); tap2(x0 + y1 + z0, c010, c110);
                tap2(x0 + y0 + z1, c001, c101); tap2(x0 + y1 + z1, c011, c111);
                if (!pair) {
                    c100 = tap(x1 + y0 + z0); c110 = tap(x1 + y1 + z0); c101 = tap(x1 + y0 + z1); c111 = tap(x1 + y1 + z1);
                }
            }
            const float c00 = tri_lerp(c000, c100, ax), c10 = tri_lerp(c010, c110, ax);
            const float c01 = tri_lerp(c001, c101, ax), c11 = tri_lerp(c011, c111, ax);
            const float e0 = tri_lerp(c00, c10, ay), e1 = tri_lerp(c01, c11, ay);
            return tri_lerp(e0, e1, az);
        };
        // cartesianToTextureCoord (VolumeRenderer.cs:175-192), as the generic kernel computes it
        auto texcoord = [&](float qx, float qy, float qz, float &tcx, float &tcy, float &tcz) {
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
            if (P.view_top == 1) { tcx = ux; tcy = uzr; tcz = uy; }
            else if (P.view_bottom == 1) { tcx = ux; tcy = uz; tcz = 1.0f - uy; }
            else { tcx = ux; tcy = uy; tcz = uz; }
        };
        auto nearest_index = [&](float tc, float fdim, int n) -> int { return clampi(floor_to_int_sat(tc * fdim), 0, n - 1); };
        auto sample_at = [&](float tcx, float tcy, float tcz) -> float {
            if (FILTER == 0)
                return voxel(nearest_index(tcx, P.fdim[0], P.nx), nearest_index(tcy, P.fdim[1], P.ny), nearest_index(tcz, P.fdim[2], P.nz));
            return trilinear(tcx * P.fdim[0] - 0.5f, tcy * P.fdim[1] - 0.5f, tcz * P.fdim[2] - 0.5f);
        };

        const float EPSILON = 0.000001f;
        const float sx = ray.ox + ray.dx * t_min, sy = ray.oy + ray.dy * t_min, sz = ray.oz + ray.dz * t_min;
        const float p0x = sx + ray.dx * EPSILON, p0y = sy + ray.dy * EPSILON, p0z = sz + ray.dz * EPSILON;
        const float dsx = ray.dx * P.step, dsy = ray.dy * P.step, dsz = ray.dz * P.step;
        float qx = p0x, qy = p0y, qz = p0z;          // q_i
        float rx = p0x, ry = p0y, rz = p0z;          // q_{i-1}
        float s_prev = 0.0f, s_hit = 0.0f;
        bool prev_fetched = false, hit = false;
        int i = 0;
        uint32_t cell = 0xffffffffu;
        bool cell_empty = false;
        // ---- the march: the composite mode's positions and box-exit test (without its dest.a term), no window, no compositing
        for (; i < P.max_steps; i++) {
            if (P.accum == 1) {
                const float fi = (float)i;
                qx = p0x + fi * dsx; qy = p0y + fi * dsy; qz = p0z + fi * dsz;
            }
            float tcx, tcy, tcz;
            texcoord(qx, qy, qz, tcx, tcy, tcz);
            if (tcx > 1.0f || tcy > 1.0f || tcz > 1.0f || tcx < 0.0f || tcy < 0.0f || tcz < 0.0f) break;
            bool fetch = true;
            if (SKIP) {
                // the sample's cell: its NEAREST voxel (TRILINEAR: its lower tap), >> 3
                int ci, cj, ck;
                if (FILTER == 0) {
                    ci = nearest_index(tcx, P.fdim[0], P.nx); cj = nearest_index(tcy, P.fdim[1], P.ny); ck = nearest_index(tcz, P.fdim[2], P.nz);
                } else {
                    ci = clampi((int)floorf(tcx * P.fdim[0] - 0.5f), 0, P.nx - 1);
                    cj = clampi((int)floorf(tcy * P.fdim[1] - 0.5f), 0, P.ny - 1);
                    ck = clampi((int)floorf(tcz * P.fdim[2] - 0.5f), 0, P.nz - 1);
                }
                const uint32_t c = ((uint32_t)ci >> 3) + (uint32_t)P.cnx * (((uint32_t)cj >> 3) + (uint32_t)P.cny * ((uint32_t)ck >> 3));
                if (c != cell) {
                    cell = c;
                    cell_empty = (float)grid[c] < iso_s;
                }
                fetch = !cell_empty;
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
                    texcoord(rx, ry, rz, tcx, tcy, tcz);
                    s_prev = sample_at(tcx, tcy, tcz);
                }
                const float f = (iso_s - s_prev) / (s_hit - s_prev);
                hx = rx + f * (qx - rx); hy = ry + f * (qy - ry); hz = rz + f * (qz - rz);
            }
            // ---- gradient: central differences of the same sampler at h, +-1 voxel per volume axis, clamped to the edge
            float tcx, tcy, tcz;
            texcoord(hx, hy, hz, tcx, tcy, tcz);
            float gx, gy, gz;
            if (FILTER == 0) {
                const int vi = nearest_index(tcx, P.fdim[0], P.nx), vj = nearest_index(tcy, P.fdim[1], P.ny), vk = nearest_index(tcz, P.fdim[2], P.nz);
                gx = voxel(clampi(vi + 1, 0, P.nx - 1), vj, vk) - voxel(clampi(vi - 1, 0, P.nx - 1), vj, vk);
                gy = voxel(vi, clampi(vj + 1, 0, P.ny - 1), vk) - voxel(vi, clampi(vj - 1, 0, P.ny - 1), vk);
                gz = voxel(vi, vj, clampi(vk + 1, 0, P.nz - 1)) - voxel(vi, vj, clampi(vk - 1, 0, P.nz - 1));
            } else {
                const float u = tcx * P.fdim[0] - 0.5f, v = tcy * P.fdim[1] - 0.5f, w = tcz * P.fdim[2] - 0.5f;
                gx = trilinear(u + 1.0f, v, w) - trilinear(u - 1.0f, v, w);
                gy = trilinear(u, v + 1.0f, w) - trilinear(u, v - 1.0f, w);
                gz = trilinear(u, v, w + 1.0f) - trilinear(u, v, w - 1.0f);
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
                float s = gl_min(gl_max(iso_s, P.fmin), P.fmax);
                if (P.fden == 0.0f) s = 0.0f;
                else if (s <= P.fmax && s >= P.fmin) s = (s - P.fmin) / P.fden;
                const int idx = clampi(floor_to_int_sat(s * (float)(P.tf_len - 1) + 0.5f), 0, P.tf_len - 1);
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

static inline unsigned iso_padded_blocks(unsigned tiles_x, unsigned tiles_y)
{
    // as vr_kernels.hip: every XCD gets ceil(tiles_y / 8) tile rows' worth of slots; extras are padding
    return ((tiles_y + 7u) / 8u) * tiles_x * 8u;
}

template <typename VoxelT, int LAYOUT, int FILTER, bool SKIP>
static hipError_t launch_iso(const FrameParams &P, const LaunchConfig &L, const IsoArgs &A, const void *vol, const float4 *tf, float4 *fb,
                             uint32_t *spp, unsigned tiles_x, unsigned tiles_y, hipStream_t st)
{
    const int div = L.divmode_tc == DIV_EXACT ? DIV_EXACT : DIV_CERT;
    const dim3 grid(iso_padded_blocks(tiles_x, tiles_y)), block(256);
    if (L.big_offsets)
        hipLaunchKernelGGL((raymarch_iso_kernel<VoxelT, LAYOUT, FILTER, SKIP, true>), grid, block, 0, st, P, div, 0u, (const VoxelT *)vol, tf,
                           fb, spp, A.depth, A.skip_grid, A.iso_s, tiles_x, tiles_y);
    else
        hipLaunchKernelGGL((raymarch_iso_kernel<VoxelT, LAYOUT, FILTER, SKIP, false>), grid, block, 0, st, P, div, (uint32_t)L.vol_bytes32,
                           (const VoxelT *)vol, tf, fb, spp, A.depth, A.skip_grid, A.iso_s, tiles_x, tiles_y);
    return hipGetLastError();
}

template <typename VoxelT>
static hipError_t launch_iso_type(const FrameParams &P, const LaunchConfig &L, const IsoArgs &A, const void *vol, const float4 *tf,
                                  float4 *fb, uint32_t *spp, hipStream_t st)
{
    const int rows = launch_local_rows(P);
    const unsigned tiles_x = (unsigned)((P.img_w + 15) / 16), tiles_y = (unsigned)((rows + 15) / 16);
    const bool skip = A.skip_grid != nullptr;
#define VR_ISO_L(LAY)                                                                                                              \
    if (L.filter == 0) return skip ? launch_iso<VoxelT, LAY, 0, true>(P, L, A, vol, tf, fb, spp, tiles_x, tiles_y, st)             \
                                   : launch_iso<VoxelT, LAY, 0, false>(P, L, A, vol, tf, fb, spp, tiles_x, tiles_y, st);           \
    return skip ? launch_iso<VoxelT, LAY, 1, true>(P, L, A, vol, tf, fb, spp, tiles_x, tiles_y, st)                                \
                : launch_iso<VoxelT, LAY, 1, false>(P, L, A, vol, tf, fb, spp, tiles_x, tiles_y, st);
    if (L.layout == 0) { VR_ISO_L(0) }
    VR_ISO_L(1)
#undef VR_ISO_L
}

#define VR_ISO_ARGS const FrameParams &P, const LaunchConfig &L, const IsoArgs &A, const void *vol, const float4 *tf, float4 *fb, uint32_t *spp, hipStream_t st
#if VR_ISO_TU == 0 || VR_ISO_TU == -1
hipError_t launch_iso_u8(VR_ISO_ARGS) { return launch_iso_type<uint8_t>(P, L, A, vol, tf, fb, spp, st); }
#endif
#if VR_ISO_TU == 1 || VR_ISO_TU == -1
hipError_t launch_iso_u16(VR_ISO_ARGS) { return launch_iso_type<uint16_t>(P, L, A, vol, tf, fb, spp, st); }
#endif

// one empty kernel per unit: launching it makes the runtime inflate and load that unit's code object
#if VR_ISO_TU >= 0
#define VR_ISO_CAT2(a, b) a##b
#define VR_ISO_CAT(a, b) VR_ISO_CAT2(a, b)
__global__ void VR_ISO_CAT(warm_kernel_iso, VR_ISO_TU)() {}
hipError_t VR_ISO_CAT(launch_warm_iso_tu, VR_ISO_TU)(hipStream_t st)
{
    hipLaunchKernelGGL(VR_ISO_CAT(warm_kernel_iso, VR_ISO_TU), dim3(1), dim3(64), 0, st);
    return hipGetLastError();
}
#endif

// the unit of 8-bit volumes also carries the entry points
#if VR_ISO_TU == 0 || VR_ISO_TU == -1
#if VR_ISO_TU == 0
hipError_t launch_iso_u16(VR_ISO_ARGS);
hipError_t launch_warm_iso_tu1(hipStream_t st);
#endif

hipError_t launch_raymarch_iso(VR_ISO_ARGS, const char **kernel_name)
{
    if (kernel_name) *kernel_name = "raymarch_iso_kernel";
    if (launch_local_rows(P) <= 0 || P.img_w <= 0) return hipSuccess;
    if (!A.depth) return hipErrorInvalidValue;
    return L.bytes_per_voxel == 1 ? launch_iso_u8(P, L, A, vol, tf, fb, spp, st) : launch_iso_u16(P, L, A, vol, tf, fb, spp, st);
}

hipError_t launch_warm_iso(hipStream_t st)
{
#if VR_ISO_TU == 0
    hipError_t e = launch_warm_iso_tu0(st);
    if (e == hipSuccess) e = launch_warm_iso_tu1(st);
    return e;
#else
    (void)st;
    return hipSuccess;
#endif
}
#endif
#undef VR_ISO_ARGS

}  // namespace vr
