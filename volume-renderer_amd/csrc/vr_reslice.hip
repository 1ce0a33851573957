// vr_reslice.hip -- the multi-planar reslice kernel (vr_set_reslice): per pixel a short line of n samples across a plane
// given in voxel index coordinates, reduced to its maximum, minimum or mean (thick-slab MIP / MinIP / average; n = 1 is a
// plain slice), windowed like the composite mode, and the raw value stored for read-back.  The definition, step by step, is
// in include/vr_core.h and DESIGN.md section 1; tests/reslice_ref/reslice_ref.c restates it on the CPU and
// tests/test_reslice_gpu.py holds this kernel to it bit for bit.
//
// Its own translation units (VR_RESLICE_TU = 0: 8-bit volumes and the entry point, 1: 16-bit volumes; the build always sets it, and
// VR_CODE_UNIT registers each for the pre-load), like vr_iso.hip; launched through mode_dispatch.h (MODE is its extra axis): the
// vr_kernels.hip units, FrameParams and LaunchConfig are untouched by the mode; the plane, the slab and the values target
// are extra kernel arguments.  Arithmetic contract as in vr_kernels.hip: one correctly rounded fp32 operation per step,
// nothing contracted (-ffp-contract=off); the only fused operations are explicit: TRILINEAR's lerps (tri_lerp) and the
// certified window division (div_cert).
//
// Shape: the isosurface kernel's -- one pixel per lane, 8x8 pixels per wavefront, 16x16-pixel tiles of four wavefronts dealt
// to the XCDs by tile_of_block().  A wavefront's 64 lanes sample a compact 8x8 patch of the plane, about 2x2 bricks of 4^3
// per slab step, so neighbouring lanes share cache lines.  The slab loop is unrolled by 4: four positions, their loads, then
// the reduction in k order -- several misses in flight per lane without changing the order of the sum.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mode_dispatch.h"
#include "vr_code_unit.h"
#include "vr_sampler.h"
#include "vr_reslice.h"

#ifndef VR_RESLICE_TU
#error "VR_RESLICE_TU: the unit number comes from the build"
#endif

namespace vr {

template <typename VoxelT, int LAYOUT, int FILTER, int MODE, bool BIG>
__global__ __launch_bounds__(256) void reslice_kernel(const FrameParams P, const ResliceGeom G, const int n, const int divmode,
                                                      const int hu_offset, const uint32_t vol_bytes, const VoxelT *__restrict__ vol,
                                                      const float4 *__restrict__ tf, float4 *__restrict__ fb, uint32_t *__restrict__ spp,
                                                      float *__restrict__ values, const unsigned tiles_x, const unsigned tiles_y)
{
    unsigned tx, ty;
    tile_of_block(blockIdx.x, tiles_x, tiles_y, tx, ty);
    if (tx == 0xffffffffu) return;
    int lx, ly, px, py;
    if (!tile_pixel(P, tx, ty, lx, ly, px, py)) return;

    // NEAREST at a voxel inside the volume; TRILINEAR at continuous voxel coordinates (u, v, w)
    const VolumeSampler<VoxelT, LAYOUT, BIG> S(P, vol, vol_bytes);

    // ---- the line: p = (o + X * du) + Y * dv per component, q_k = p + c_k * dw, c_k = (2k - (n - 1)) / 2 (exact)
    const float X = (float)px, Y = (float)py;
    const float pxv = (G.o[0] + X * G.du[0]) + Y * G.dv[0];
    const float pyv = (G.o[1] + X * G.du[1]) + Y * G.dv[1];
    const float pzv = (G.o[2] + X * G.du[2]) + Y * G.dv[2];
    float m = MODE == 0 ? -__builtin_inff() : __builtin_inff(), acc = 0.0f;
    uint32_t cnt = 0;
    for (int k0 = 0; k0 < n; k0 += 4) {
        // four positions and their inside tests; a sample outside (or past n) is sampled at voxel 0 and not taken, so the four
        // loads need no branch of their own
        float qx[4], qy[4], qz[4];
        bool in[4];
        bool any = false;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int k = k0 + j;
            const float c = (float)(2 * k - (n - 1)) * 0.5f;
            const float x = pxv + c * G.dw[0], y = pyv + c * G.dw[1], z = pzv + c * G.dw[2];
            const float rx = x + 0.5f, ry = y + 0.5f, rz = z + 0.5f;
            in[j] = k < n && rx >= 0.0f && rx < P.fdim[0] && ry >= 0.0f && ry < P.fdim[1] && rz >= 0.0f && rz < P.fdim[2];
            any = any || in[j];
            if (FILTER == 0) { qx[j] = in[j] ? rx : 0.0f; qy[j] = in[j] ? ry : 0.0f; qz[j] = in[j] ? rz : 0.0f; }
            else { qx[j] = in[j] ? x : 0.0f; qy[j] = in[j] ? y : 0.0f; qz[j] = in[j] ? z : 0.0f; }
        }
        if (!any) continue;
        float s[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (FILTER == 0) s[j] = S.voxel((int)qx[j], (int)qy[j], (int)qz[j]);        // r in [0, dim): truncation is the floor
            else s[j] = S.trilinear(qx[j], qy[j], qz[j]);
        }
        // ---- the reduction, in increasing k
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (!in[j]) continue;
            cnt++;
            if (MODE == 0) { if (s[j] > m) m = s[j]; }
            else if (MODE == 1) { if (s[j] < m) m = s[j]; }
            else acc = acc + s[j];
        }
    }

    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, c3 = 0.0f;
    float out = __uint_as_float(0x7fc00000u);          // the canonical quiet NaN: no inside sample
    if (cnt > 0) {
        const float value = MODE == 2 ? acc / (float)cnt : m;
        out = hu_offset ? value - 1000.0f : value;
        // window (the composite mode's rule; max == min: 0)
        const float v = window_map(P, value, divmode);
        c0 = v; c1 = v; c2 = v; c3 = 1.0f;
        if (P.tf_len > 1) {
            const int idx = tf_index(P, v);
            const float4 t = tf[idx];
            c0 = t.x; c1 = t.y; c2 = t.z;
        }
    }
    const size_t pix = (size_t)(P.fb_compact ? ly : py) * (size_t)P.img_w + (size_t)px;
    store_pixel(P, fb, pix, c0, c1, c2, c3);
    values[pix] = out;
    if (spp) spp[pix] = cnt;
}

template <typename VoxelT>
static hipError_t launch_rs_type(const FrameParams &P, const LaunchConfig &L, const ResliceArgs &A, const void *vol, const float4 *tf,
                                 float4 *fb, uint32_t *spp, hipStream_t st)
{
    const Tiles16 t = launch_tiles16(P);
    const int div = window_divmode(L);
    const dim3 grid(padded_blocks(t.x, t.y)), block(256);
    return dispatch_mode(L, IntAxis<3>{A.mode}, [&](auto LAY, auto FIL, auto MODE, auto BIG) {
        hipLaunchKernelGGL((reslice_kernel<VoxelT, LAY(), FIL(), MODE(), BIG()>), grid, block, 0, st, P, A.g, A.n, div, A.hu_offset,
                           BIG() ? 0u : (uint32_t)L.vol_bytes32, (const VoxelT *)vol, tf, fb, spp, A.values, t.x, t.y);
        return hipGetLastError();
    });
}

VR_CODE_UNIT(reslice, VR_RESLICE_TU, "reslice", WARM_LOAD_SHADER)

#define VR_RESLICE_ARGS const FrameParams &P, const LaunchConfig &L, const ResliceArgs &A, const void *vol, const float4 *tf, float4 *fb, uint32_t *spp, hipStream_t st
#if VR_RESLICE_TU == 1
hipError_t launch_reslice_u16(VR_RESLICE_ARGS) { return launch_rs_type<uint16_t>(P, L, A, vol, tf, fb, spp, st); }
#else
// the unit of 8-bit volumes also carries the entry point
hipError_t launch_reslice_u16(VR_RESLICE_ARGS);

hipError_t launch_reslice(VR_RESLICE_ARGS, const char **kernel_name)
{
    if (kernel_name) *kernel_name = "reslice_kernel";
    if (launch_local_rows(P) <= 0 || P.img_w <= 0) return hipSuccess;
    if (!A.values || A.n < 1 || A.n > 1024 || A.mode < 0 || A.mode > 2) return hipErrorInvalidValue;
    return L.bytes_per_voxel == 1 ? launch_rs_type<uint8_t>(P, L, A, vol, tf, fb, spp, st) : launch_reslice_u16(P, L, A, vol, tf, fb, spp, st);
}
#endif
#undef VR_RESLICE_ARGS

}  // namespace vr
