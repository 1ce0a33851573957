// vr_sampler.h -- the volume sampler and the per-pixel scaffold shared by the one-pixel-per-lane kernels on 16x16-pixel tiles
// (vr_generic.hip, vr_iso.hip, vr_reslice.hip, vr_shade.hip): the tile-to-pixel mapping, NEAREST and TRILINEAR fetches, the texture
// coordinates, the window map and the transfer-function index.  Arithmetic contract as in vr_kernels.hip.  What only the
// isosurface and the shading kernel share (ray start, skip cell) is in vr_march.h; their launch scaffold is mode_dispatch.h.
#pragma once
#include "vr_device.h"

namespace vr {

// The pixel of this lane in tile (tx, ty): 8x8 pixels per wavefront, four wavefronts per tile.  (lx, ly) = local position,
// (px, py) = position in the image: local row -> global row (contiguous shard or cyclic stripes).  false = outside the launch.
__device__ __forceinline__ bool tile_pixel(const FrameParams &P, unsigned tx, unsigned ty, int &lx, int &ly, int &px, int &py)
{
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    lx = (int)(tx * 16u + (wave & 1u) * 8u + (lane & 7u));
    ly = (int)(ty * 16u + (wave >> 1) * 8u + (lane >> 3));
    px = lx;
    if (P.stripe_count > 1) {
        const int s = ly / P.stripe_rows, r = ly % P.stripe_rows;
        py = (s * P.stripe_count + P.stripe_index) * P.stripe_rows + r;
    } else {
        py = P.row_begin + ly;
    }
    return !(px >= P.col_lim || py >= P.row_lim || py >= P.row_end);
}

// BIG = false: 32-bit voxel offsets through a bounds-checked buffer resource (VoxelAddr / VoxelFetch); the eight taps of
// TRILINEAR share their per-axis address terms.  BIG = true: 64-bit offsets, plain global loads (fetch_voxel).
template <typename VoxelT, int LAYOUT, bool BIG>
struct VolumeSampler {
    const FrameParams &P;
    const VoxelT *__restrict__ vol;
    const __amdgpu_buffer_rsrc_t rs;

    __device__ __forceinline__ VolumeSampler(const FrameParams &P_, const VoxelT *__restrict__ vol_, uint32_t vol_bytes)
        : P(P_), vol(vol_), rs(__builtin_amdgcn_make_buffer_rsrc((void *)vol_, 0, BIG ? 0 : (int)pair_load_extent(vol_bytes), 0x00020000))
    {
    }

    // per-axis terms of VoxelAddr<LAYOUT, false>::at(i, j, k) = X(i) + Y(j) + Z(k)  (mod 2^32)
    __device__ __forceinline__ uint32_t term_x(int i) const
    {
        return LAYOUT == 0 ? (uint32_t)i : mad_u24((uint32_t)i >> BRICK_LX, 64u - (uint32_t)BRICK_X, (uint32_t)i);
    }
    __device__ __forceinline__ uint32_t term_y(int j) const
    {
        if (LAYOUT == 0) return mad_u24((uint32_t)j, (uint32_t)P.nx, 0u);
        return mad_u24(BRICK_LY ? (uint32_t)j >> BRICK_LY : (uint32_t)j, P.bstride_y, BRICK_LY ? (uint32_t)j << BRICK_LX : 0u);
    }
    __device__ __forceinline__ uint32_t term_z(int k) const
    {
        if (LAYOUT == 0) return mad_u24(mad_u24((uint32_t)k, (uint32_t)P.ny, 0u), (uint32_t)P.nx, 0u);
        return mad_u24(BRICK_LZ ? (uint32_t)k >> BRICK_LZ : (uint32_t)k, P.bstride_z, BRICK_LZ ? (uint32_t)k << (BRICK_LX + BRICK_LY) : 0u);
    }
    __device__ __forceinline__ float tap(uint32_t off) const { return (float)VoxelFetch<VoxelT, false>::load(vol, rs, off); }
    // the tap at `off` together with the next storage element, in one load (bounds-checked: the last element of the buffer
    // reads 0 there)
    __device__ __forceinline__ void tap2(uint32_t off, float &lo, float &hi) const
    {
        if (sizeof(VoxelT) == 1) {
            const uint32_t q = (uint32_t)(uint16_t)__builtin_amdgcn_raw_buffer_load_b16(rs, (int)off, 0, 0);
            lo = (float)(q & 0xffu); hi = (float)(q >> 8);
        } else {
            const uint32_t q = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs, (int)(off << 1), 0, 0);
            lo = (float)(q & 0xffffu); hi = (float)(q >> 16);
        }
    }
    // NEAREST: voxel (i, j, k), indices already clamped
    __device__ __forceinline__ float voxel(int i, int j, int k) const
    {
        return BIG ? fetch_voxel<VoxelT, LAYOUT>(P, vol, i, j, k) : tap(term_x(i) + term_y(j) + term_z(k));
    }
    // TRILINEAR at the sampler's own continuous coordinates (u, v, w) = tc * dim - 0.5: GL's linear rule, taps clamped to
    // the edge, x then y then z, each lerp one fma
    __device__ __forceinline__ float trilinear(float u, float v, float w) const
    {
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
            // the two x-neighbours of a tap pair are adjacent in memory unless i0 is the last
            // voxel of its brick row (or of the volume): every lane fetches its x0 tap together
            // with the next storage element in one load (tap2), and only the lanes whose x1 lies
            // elsewhere fetch it again
            const bool pair = i1 == i0 + 1 && (LAYOUT == 0 || ((uint32_t)i0 & (BRICK_X - 1u)) != BRICK_X - 1u);
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
    }
};

// cartesianToTextureCoord (VolumeRenderer.cs:175-192): box position q -> texture coordinates (generic and isosurface kernels).
// The shading kernel keeps the same lines inline in its loop: called from there, this function changes its compiled code.
__device__ __forceinline__ void texcoord(const FrameParams &P, int divmode, float qx, float qy, float qz, float &tcx, float &tcy, float &tcz)
{
    float ux = qx + P.half[0], uy = qy + P.half[1], uz = qz + P.half[2];
    if (divmode == DIV_CERT) {
        ux = div_cert(ux, P.ext[0], P.rext[0]);
        uy = div_cert(uy, P.ext[1], P.rext[1]);
        uz = div_cert(uz, P.ext[2], P.rext[2]);
    } else {
        ux = ux / P.ext[0]; uy = uy / P.ext[1]; uz = uz / P.ext[2];
    }
    const float uzr = uz;   // z before the flip of :185
    uz = 1.0f - uz;
    if (P.view_top == 1) { tcx = ux; tcy = uzr; tcz = uy; }   // 1 - (1 - z) as the GL compiles it: z
    else if (P.view_bottom == 1) { tcx = ux; tcy = uz; tcz = 1.0f - uy; }
    else { tcx = ux; tcy = uy; tcz = uz; }
}

// window (VolumeRenderer.cs:122-124; Q4: max == min defined as 0); divmode = DIV_CERT: the division certified like the
// composite kernels' (kept an int: as a bool it changes the compiled shading kernel)
__device__ __forceinline__ float window_map(const FrameParams &P, float s, int divmode)
{
    s = gl_min(gl_max(s, P.fmin), P.fmax);
    if (P.fden == 0.0f) s = 0.0f;
    else if (s <= P.fmax && s >= P.fmin) s = divmode == DIV_CERT ? div_cert(s - P.fmin, P.fden, P.rden) : (s - P.fmin) / P.fden;
    return s;
}

// transfer-function entry of a windowed value: round to nearest, clamped
__device__ __forceinline__ int tf_index(const FrameParams &P, float s)
{
    return clampi(floor_to_int_sat(s * (float)(P.tf_len - 1) + 0.5f), 0, P.tf_len - 1);
}

}  // namespace vr
