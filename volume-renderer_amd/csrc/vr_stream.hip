// vr_stream.hip -- the ray-ordered sample stream of a still view (vr_set_ray_stream).
//
// Which voxel each sample of a NEAREST frame reads depends on the volume and the ray geometry only -- not on the window, the
// opacity scale, the transfer function or MIP.  While the geometry stands still (RendererCore: rayGeometryKey), the voxels the
// shader's loop reads are kept in HBM in ray order, and a frame is rendered by streaming them: one coalesced load per lane per
// G = 4 samples, then classification and compositing with the shader's own operations in the shader's order.  Another speed
// copy that holds the same voxels (like the 12-bit packed copy): frames are bit-identical, and every replayed frame still
// classifies and composites every sample, so window, alpha, transfer-function and MIP changes render from the same stream.
//
// The replay loop (raymarch_stream_kernel): a wavefront replays one block and keeps DEPTH loaded groups beyond the DEPTH it
// composites; the instances without a classification table run as one-wavefront workgroups, eight per tile.  The grey ramp of
// a large packed stream (vr_set_ray_stream_table) is classified through an LDS table whose reads are asked for a group ahead.
//
// Build (once per still view; VolumeCopies::ensureRayStream): stream_record_kernel<COUNT> writes the geometric sample count n
// of every ray, a device scan turns the blocks' padded lengths into 64-bit element offsets, the host reads the total back --
// ONE blocking 8-byte read-back per build -- allocates, and stream_record_kernel<!COUNT> writes the voxels.
// Layout: a block is one 8x8-pixel wavefront tile; n_max(block) = max n over its lanes rounded up to G; sample i of lane l sits
// at offsets[block] + (i / G) * 64 * G + l * G + i % G: a wavefront instruction reads 512 (u16) / 256 (u8) contiguous bytes.
//
// Its own translation units (VR_STREAM_TU = 0: 8-bit volumes, the scan and the entry points; 1: 16-bit volumes; 2: 16-bit
// volumes in the 12-bit packed format, below and vr_stream_pack.h), like
// vr_iso.hip: the vr_kernels.hip units are untouched, a frame whose camera moves runs the machine code it always ran.  Shared
// with them is what vr_device.h offers; the classification table, classify and accumulate are restated from vr_fast.hip, each
// with the shader lines it implements.  Arithmetic contract as in vr_kernels.hip (-ffp-contract=off, one rounding per step).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "vr_code_unit.h"
#include "vr_device.h"
#include "vr_lds_dma.h"
#include "vr_stream.h"

#ifndef VR_STREAM_TU
#error "VR_STREAM_TU: the unit number comes from the build"
#endif
// groups of G samples a lane keeps in flight beyond the ones it composites, and plain (0) or non-temporal (1) stream loads:
// measured alternatives in docs/lab-notebook.md, "Ray-ordered sample stream: first measurements"
#ifndef VR_STREAM_DEPTH
#define VR_STREAM_DEPTH 4
#endif
#ifndef VR_STREAM_NT
#define VR_STREAM_NT 1
#endif
// the same for the packed format, in groups of 8 samples (12 bytes): measured in docs/lab-notebook.md, "Ray stream: 12-bit samples"
#ifndef VR_STREAM12_DEPTH
#define VR_STREAM12_DEPTH 4
#endif
// threads per workgroup of the table-less instances: 64, 128, 256, or 512 (one tile per workgroup, like the instances with a
// table): measured in docs/lab-notebook.md, "Ray stream: wave-uniform replay"
#ifndef VR_STREAM_WG
#define VR_STREAM_WG 64
#endif
static_assert(VR_STREAM_WG == 64 || VR_STREAM_WG == 128 || VR_STREAM_WG == 256 || VR_STREAM_WG == 512,
              "a tile's eight wavefronts are split into 8, 4, 2 or 1 workgroups");
// The hybrid classification of the grey ramp (vr_set_ray_stream_table; TSHARE of raymarch_stream_kernel): of every four samples
// VR_STREAM_TSHARE (1, 2 or 4) are classified through the 32 KiB LDS table of (c, a), one ds_read_b64 each, asked for one loaded
// group ahead, and the rest arithmetically; VR_STREAM_TWG threads per workgroup share one table (512: one per tile, 256: two
// workgroups per tile, four of which fit a CU's LDS).  Measured: every share at both sizes, and a 16 KiB table of s alone, in
// docs/lab-notebook.md, "Ray stream: a share of the samples classified through LDS" -- all four through the table, from
// 256-thread workgroups, is what the headline's stream, the shard's and the 8-bit shape's replay fastest from; no share gains
// on the unpacked cfg2 stream
#ifndef VR_STREAM_TSHARE
#define VR_STREAM_TSHARE 4
#endif
#ifndef VR_STREAM_TWG
#define VR_STREAM_TWG 256
#endif
static_assert(VR_STREAM_TSHARE == 1 || VR_STREAM_TSHARE == 2 || VR_STREAM_TSHARE == 4, "table samples per four");
static_assert(VR_STREAM_TWG == 256 || VR_STREAM_TWG == 512, "a table is shared by four or eight wavefronts of a tile");

namespace vr {

constexpr unsigned STREAM_G = kStreamGroup, STREAM_BLOCK_ELEMS = 64u * STREAM_G;
static_assert(STREAM_G == 4, "a group is one 8-byte (u16) / 4-byte (u8) load: the packing below spells out four samples");
// The packed format (vr_stream_pack.h; 16-bit volumes whose exact range spans at most 4095): G = 8 samples of 12 bits are one
// 12-byte load, a wavefront instruction reads 768 contiguous bytes.  A block's element offset o is a multiple of 512, its byte
// offset is o / 2 * 3.
constexpr unsigned STREAM12_G = kStreamGroup12, STREAM12_BLOCK_ELEMS = 64u * STREAM12_G;
static_assert(STREAM12_G == 2 * STREAM_G, "a packed group is consumed as two groups of four");

// ------------------------------------------------------------------ build: count / record
// One pixel per lane, 8x8 pixels per wavefront (= one stream block), four blocks per workgroup, over the launch's local rows:
// stripes, compact targets and the Q1 limits as raymarch_fast_kernel maps them (vr_fast.hip:80-91).  The shader's loop,
// literally: position mapping, bounds test and clamped voxel index of checked_step (vr_fast.hip:393-410) -- with no opacity
// test and no compositing.  COUNT: n = iterations until a bound test fails (<= max_steps, fits 16 bits).  !COUNT: the same
// positions once more, the bound tests replaced by i < n of the count pass, the fetches of 8 samples issued together (the
// positions do not depend on the data); always from the resident volume, never from the packed copy.
// `group` (COUNT): the group size n_max is rounded up to.  PACK (!COUNT): the packed format -- voxel - base (P.pk12_base) in 12
// bits, three dwords per lane per group of 8, 0 in a padded slot.
template <typename VoxelT, int LAYOUT, bool BIG, bool COUNT, bool PACK = false>
__global__ __launch_bounds__(256) void stream_record_kernel(const FrameParams P, const int divmode, const int view,
                                                            const VoxelT *__restrict__ vol, const uint32_t vol_bytes,
                                                            uint16_t *__restrict__ counts, uint32_t *__restrict__ block_elems,
                                                            const uint64_t *__restrict__ offsets, VoxelT *__restrict__ samples,
                                                            const unsigned blocks_x, const unsigned blocks, const unsigned group)
{
    static_assert(!PACK || (!COUNT && sizeof(VoxelT) == 2), "the packed format holds 16-bit voxels");
    const unsigned lane = threadIdx.x & 63u;
    const unsigned sb = (unsigned)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    if (sb >= blocks) return;
    const unsigned bx = sb % blocks_x, by = sb / blocks_x;
    const int lx = (int)(bx * 8u + (lane & 7u)), ly = (int)(by * 8u + (lane >> 3));
    const int px = lx;
    int py;
    if (P.stripe_count > 1) {
        const int s = ly / P.stripe_rows, r = ly % P.stripe_rows;
        py = (s * P.stripe_count + P.stripe_index) * P.stripe_rows + r;
    } else {
        py = P.row_begin + ly;
    }
    const bool in_image = !(px >= P.col_lim || py >= P.row_lim || py >= P.row_end);

    Ray ray = {};
    float t_min = 0.0f, t_max = 0.0f;
    bool hit = false;
    if (in_image) {
        ray = compute_ray(P, (float)px + 0.5f, (float)py + 0.5f);
        hit = intersect_ray_aabb(P, ray, t_min, t_max);
    }
    const float EPSILON = 0.000001f;
    const float sx = ray.ox + ray.dx * t_min, sy = ray.oy + ray.dy * t_min, sz = ray.oz + ray.dz * t_min;
    float x = sx + ray.dx * EPSILON, y = sy + ray.dy * EPSILON, z = sz + ray.dz * EPSILON;
    const float dsx = ray.dx * P.step, dsy = ray.dy * P.step, dsz = ray.dz * P.step;
    // cartesianToTextureCoord (VolumeRenderer.cs:175-192) as checked_step restates it; the division by run-time mode
    // (DIV_UNIT: the divisor is exactly 1; DIV_CERT: the certified quotient) -- a wave-uniform switch in a one-off kernel
    auto texcoord = [&](float ax, float ay, float az, float &tcx, float &tcy, float &tcz) {
        float ux = ax + P.half[0], uy = ay + P.half[1], uzr = az + P.half[2];   // z before the flip of :185
        if (divmode == DIV_CERT) {
            ux = div_cert(ux, P.ext[0], P.rext[0]);
            uy = div_cert(uy, P.ext[1], P.rext[1]);
            uzr = div_cert(uzr, P.ext[2], P.rext[2]);
        }
        const float uz = 1.0f - uzr;
        tcx = ux; tcy = uy; tcz = uz;
        if (view == 1) { tcy = uzr; tcz = uy; }                 // view_top
        else if (view == 2) { tcy = uz; tcz = 1.0f - uy; }      // view_bottom
    };

    if constexpr (COUNT) {
        int n = 0;
        if (hit) {
            for (; n < P.max_steps; n++) {
                float tcx, tcy, tcz;
                texcoord(x, y, z, tcx, tcy, tcz);
                if (tcx > 1.0f || tcy > 1.0f || tcz > 1.0f || tcx < 0.0f || tcy < 0.0f || tcz < 0.0f) break;
                x += dsx; y += dsy; z += dsz;
            }
        }
        counts[(size_t)sb * 64u + lane] = (uint16_t)n;
        int nmax = n;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) nmax = max(nmax, __shfl_xor(nmax, d, 64));
        if (lane == 0) block_elems[sb] = (((uint32_t)nmax + group - 1u) / group) * (64u * group);
    } else if constexpr (PACK) {
        const int n = (int)counts[(size_t)sb * 64u + lane];
        const uint64_t off = offsets[sb];
        const uint32_t ngroups = (uint32_t)((offsets[sb + 1] - off) / STREAM12_BLOCK_ELEMS);
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)vol, 0, BIG ? 0 : (int)vol_bytes, 0x00020000);
        // (the last group's last lane ends at byte (off + ngroups * 512) / 2 * 3: inside the allocation, before its slack)
        uint32_t *out = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(samples) + off / 2u * 3u) + lane * 3u;
        const uint32_t base = (uint32_t)P.pk12_base;
        for (uint32_t g = 0; g < ngroups; g++) {
            typename VoxelAddr<LAYOUT, BIG>::type a[8];
            bool live[8];
            uint32_t t[8], d[3];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                live[u] = (int)(g * STREAM12_G) + u < n;
                float tcx, tcy, tcz;
                texcoord(x, y, z, tcx, tcy, tcz);
                const int vi = max(min((int)(tcx * P.fdim[0]), P.nx - 1), 0);
                const int vj = max(min((int)(tcy * P.fdim[1]), P.ny - 1), 0);
                const int vk = max(min((int)(tcz * P.fdim[2]), P.nz - 1), 0);
                a[u] = VoxelAddr<LAYOUT, BIG>::at(P, vi, vj, vk);
                if (!live[u]) a[u] = 0;
                x += dsx; y += dsy; z += dsz;
            }
#pragma unroll
            for (int u = 0; u < 8; u++) t[u] = VoxelFetch<VoxelT, BIG>::load(vol, rs, a[u]);
            // (the mask only keeps a field inside its 12 bits should the host's range be wrong: base <= voxel <= base + 4095)
#pragma unroll
            for (int u = 0; u < 8; u++) t[u] = live[u] ? (t[u] - base) & 0xfffu : 0u;
            stream_pack12(t, d);
            uint32_t *q = out + (size_t)g * (64u * 3u);
            q[0] = d[0]; q[1] = d[1]; q[2] = d[2];
        }
    } else {
        const int n = (int)counts[(size_t)sb * 64u + lane];
        const uint64_t off = offsets[sb];
        const uint32_t ngroups = (uint32_t)((offsets[sb + 1] - off) / STREAM_BLOCK_ELEMS);
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)vol, 0, BIG ? 0 : (int)vol_bytes, 0x00020000);
        using GroupT = typename std::conditional<sizeof(VoxelT) == 2, uint2, uint32_t>::type;
        GroupT *out = reinterpret_cast<GroupT *>(samples + off) + lane;
        for (uint32_t g = 0; g < ngroups; g += 2) {
            typename VoxelAddr<LAYOUT, BIG>::type a[8];
            bool live[8];
            uint32_t t[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                live[u] = (int)(g * STREAM_G) + u < n;
                float tcx, tcy, tcz;
                texcoord(x, y, z, tcx, tcy, tcz);
                // (the count pass proved tc >= 0 for the live samples; the lower clamp only keeps a lane past its n inside the volume)
                const int vi = max(min((int)(tcx * P.fdim[0]), P.nx - 1), 0);
                const int vj = max(min((int)(tcy * P.fdim[1]), P.ny - 1), 0);
                const int vk = max(min((int)(tcz * P.fdim[2]), P.nz - 1), 0);
                a[u] = VoxelAddr<LAYOUT, BIG>::at(P, vi, vj, vk);
                // a padded slot holds voxel (0, 0, 0): a value of the volume (the replay classifies whole groups, and never composites it)
                if (!live[u]) a[u] = 0;
                x += dsx; y += dsy; z += dsz;
            }
#pragma unroll
            for (int u = 0; u < 8; u++) t[u] = VoxelFetch<VoxelT, BIG>::load(vol, rs, a[u]);
#pragma unroll
            for (int h = 0; h < 2; h++) {
                if (g + (uint32_t)h >= ngroups) break;
                const uint32_t *q = t + 4 * h;
                if constexpr (sizeof(VoxelT) == 2) out[(size_t)(g + h) * 64u] = make_uint2(q[0] | (q[1] << 16), q[2] | (q[3] << 16));
                else out[(size_t)(g + h) * 64u] = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
            }
        }
    }
}

template <typename VoxelT, int LAYOUT, bool BIG, bool PACK>
static hipError_t launch_record_instance(const FrameParams &P, const LaunchConfig &L, const void *vol, uint16_t *counts,
                                         uint32_t *block_elems, const uint64_t *offsets, void *samples, unsigned group, hipStream_t st)
{
    const int rows = launch_local_rows(P);
    if (rows <= 0 || P.img_w <= 0) return hipSuccess;
    const StreamGrid g = streamGrid(P.img_w, rows);
    const int view = P.view_top == 1 ? 1 : (P.view_bottom == 1 ? 2 : 0);
    const dim3 grid((g.blocks + 3u) / 4u), block(256);
    if constexpr (PACK) {
        if (samples == nullptr) return hipErrorInvalidValue;
        hipLaunchKernelGGL((stream_record_kernel<VoxelT, LAYOUT, BIG, false, true>), grid, block, 0, st, P, L.divmode_tc, view, (const VoxelT *)vol,
                           (uint32_t)L.vol_bytes32, counts, block_elems, offsets, (VoxelT *)samples, g.blocks_x, g.blocks, group);
    } else if (samples == nullptr)
        hipLaunchKernelGGL((stream_record_kernel<VoxelT, LAYOUT, BIG, true>), grid, block, 0, st, P, L.divmode_tc, view, (const VoxelT *)vol,
                           (uint32_t)L.vol_bytes32, counts, block_elems, offsets, (VoxelT *)nullptr, g.blocks_x, g.blocks, group);
    else
        hipLaunchKernelGGL((stream_record_kernel<VoxelT, LAYOUT, BIG, false>), grid, block, 0, st, P, L.divmode_tc, view, (const VoxelT *)vol,
                           (uint32_t)L.vol_bytes32, counts, block_elems, offsets, (VoxelT *)samples, g.blocks_x, g.blocks, group);
    return hipGetLastError();
}

template <typename VoxelT, bool PACK = false>
static hipError_t launch_record_type(const FrameParams &P, const LaunchConfig &L, const void *vol, uint16_t *counts, uint32_t *block_elems,
                                     const uint64_t *offsets, void *samples, unsigned group, hipStream_t st)
{
    if (L.divmode_tc == DIV_EXACT) return hipErrorInvalidValue;      // (not a fast-path frame: the host never asks)
    if (L.layout == 0)
        return L.big_offsets ? launch_record_instance<VoxelT, 0, true, PACK>(P, L, vol, counts, block_elems, offsets, samples, group, st)
                             : launch_record_instance<VoxelT, 0, false, PACK>(P, L, vol, counts, block_elems, offsets, samples, group, st);
    return L.big_offsets ? launch_record_instance<VoxelT, 1, true, PACK>(P, L, vol, counts, block_elems, offsets, samples, group, st)
                         : launch_record_instance<VoxelT, 1, false, PACK>(P, L, vol, counts, block_elems, offsets, samples, group, st);
}

// ------------------------------------------------------------------ replay
// Workgroup = 512 threads = 8 wavefronts = one 32x16-pixel tile of the fast kernel's longest-first tile table; wavefront w of
// tile (tx, ty) replays stream block (tx * 4 + (w & 3), ty * 2 + (w >> 2)).  No address tables, no barrier in the sample loop.
// An instance without a table (LUT false) uses no LDS and no barrier at all: its tiles are launched as 512 / VR_STREAM_WG
// workgroups of VR_STREAM_WG threads each, in the table's order -- a wavefront's slot is free for the next tile's as soon as
// that wavefront ends, not when the slowest of its eight does.
// MODE: raymarch_fast_kernel's (vr_fast.hip:40-47).  LUT: classification through the LDS table -- the transfer function (MODE
// >= 2) and its grey fold (MODE 0, FrameParams::tf_grey); the grey ramp is classified arithmetically (launch_replay_mode).
// NOCLAMP: the dataset's exact range lies inside the window, so clamp() is the identity.
//
// PACK ("raymarch_stream12_kernel"): the packed format.  A sample is t = voxel - base (P.pk12_base, the stream's own) and the
// base is folded into constants, so the sample loop has the unpacked format's operations after the unpack:
//  - table paths: clamp(voxel, min, max) + bias == clamp(t, min - base, max - base) + (bias + base), integers throughout;
//  - arithmetic path: the window is shifted, fmin - base and fmax - base (vr_stream_pack.h: streamBaseFoldsIntoWindow has the
//    reasoning and the bound); BASEADD, for a window beyond that bound: t + base as an integer before the convert.
typedef uint32_t stream_u32x2 __attribute__((ext_vector_type(2)));
typedef float stream_f32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t stream_u32x3 __attribute__((ext_vector_type(3)));   // (a register value only: never loaded through a pointer of this type)

template <typename VoxelT, int MODE, bool LUT, bool NOCLAMP, bool PACK = false, bool BASEADD = false, int TSHARE = 0>
__global__ __launch_bounds__(512) void raymarch_stream_kernel(const FrameParams P, const float4 *__restrict__ tf, float4 *__restrict__ fb,
                                                              const VoxelT *__restrict__ samples, const uint16_t *__restrict__ counts,
                                                              const uint64_t *__restrict__ offsets, const unsigned blocks_x,
                                                              const uint32_t *__restrict__ tile_table)
{
    static_assert(LUT || MODE < 2, "a transfer function is classified through the LDS table");
    static_assert(!NOCLAMP || (!LUT && MODE == 0), "the no-clamp specialisation exists for the grey composite's arithmetic classification");
    static_assert(!PACK || sizeof(VoxelT) == 2, "the packed format holds 16-bit voxels");
    static_assert(!BASEADD || (PACK && !LUT), "the integer add replaces the shifted window of the arithmetic path");
    static_assert(TSHARE == 0 || (!LUT && MODE < 2 && !BASEADD), "the hybrid splits the grey ramp's samples between the table and the shifted window's arithmetic");
    static_assert(TSHARE == 0 || TSHARE == 1 || TSHARE == 2 || TSHARE == 4, "table samples per four");
    constexpr unsigned G = PACK ? STREAM12_G : STREAM_G, BLOCK_ELEMS = 64u * G;
    constexpr bool TABLE = LUT || TSHARE > 0;                // the instance builds the LDS table
    __shared__ float lut[TABLE ? FAST_LUT_MAX * 2 : 4];     // 32 KiB: 4096 x (c,a) or 256 x (r,g,b,a) + index bytes
    // (a table-less instance uses no LDS and no barrier: its tile may be launched as 8 / WPB workgroups of WPB wavefronts; a
    // hybrid instance's VR_STREAM_TWG threads build and share one table)
    constexpr unsigned WPB = LUT ? 8u : (TSHARE > 0 ? (unsigned)VR_STREAM_TWG : (unsigned)VR_STREAM_WG) / 64u, SPLIT = 8u / WPB;
    const uint32_t t = tile_table[blockIdx.x / SPLIT];
    if (t == 0xffffffffu) return;                            // padding block
    const unsigned tx = t & 0xffffu, ty = t >> 16;
    const unsigned lane = threadIdx.x & 63u, wave = (blockIdx.x % SPLIT) * WPB + (threadIdx.x >> 6);
    const unsigned mx = lane & 7u, my = lane >> 3;
    const int lx = (int)(tx * kFastTileW + (wave & 3u) * 8u + mx);
    const int ly = (int)(ty * kFastTileH + (wave >> 2) * 8u + my);
    const int px = lx;
    int py;
    if (P.stripe_count > 1) {
        const int s = ly / P.stripe_rows, r = ly % P.stripe_rows;
        py = (s * P.stripe_count + P.stripe_index) * P.stripe_rows + r;
    } else {
        py = P.row_begin + ly;
    }
    const bool in_image = !(px >= P.col_lim || py >= P.row_lim || py >= P.row_end);
    const unsigned sb = (unsigned)__builtin_amdgcn_readfirstlane((int)((ty * 2u + (wave >> 2)) * blocks_x + tx * 4u + (wave & 3u)));
    const int n = (int)counts[(size_t)sb * 64u + lane];      // 0: outside the image, or the ray misses the box
    const uint64_t off = offsets[sb];
    const uint32_t ngroups = (uint32_t)((offsets[sb + 1] - off) / BLOCK_ELEMS);

    if (TABLE) {
        // the classification table, exactly as raymarch_fast_kernel builds it (vr_fast.hip:100-144); tabulated only if some ray
        // of the workgroup has a sample
        if (__syncthreads_or(n > 0 ? 1 : 0)) {
            const int ne = P.max_val - P.min_val + 1;
            for (int e = (int)threadIdx.x; e < ne; e += (int)(WPB * 64u)) {
                const float s = (float)(P.min_val + e);          // == clamp(float(texel), fmin, fmax)
                const float v = div_cert(s - P.fmin, P.fden, P.rden);
                if (MODE >= 2) {
                    // classification through the transfer function: index = round(v*(len-1)), the entry from the table below
                    int idx = floor_to_int_sat(v * (float)(P.tf_len - 1) + 0.5f);
                    idx = clampi(idx, 0, P.tf_len - 1);
                    reinterpret_cast<uint8_t *>(lut)[FAST_TF_ENTRIES * 16 + e] = (uint8_t)idx;
                } else if (MODE == 0 && P.tf_grey != 0) {
                    // a grey transfer function folded into the (c, a) table with MODE 2's own operations (vr_fast.hip:114-124)
                    int idx = floor_to_int_sat(v * (float)(P.tf_len - 1) + 0.5f);
                    idx = clampi(idx, 0, P.tf_len - 1);
                    const float4 q = tf[idx];
                    const float a = q.w * P.alpha_scale;
                    lut[2 * e + 0] = q.x * a; lut[2 * e + 1] = a;
                } else {
                    const float a = v * P.alpha_scale;           // src.a *= alpha_scale, src.rgb *= src.a (VolumeRenderer.cs:130-131)
                    lut[2 * e + 0] = v * a; lut[2 * e + 1] = a;
                }
            }
            if (MODE >= 2) {
                for (int e = (int)threadIdx.x; e < P.tf_len; e += 512) {
                    const float4 q = tf[e];
                    const float a = q.w * P.alpha_scale;
                    if (MODE == 3) {            // MIP(): s *= alpha_scale on all four channels (VolumeRenderer.cs:164)
                        lut[4 * e + 0] = q.x * P.alpha_scale; lut[4 * e + 1] = q.y * P.alpha_scale; lut[4 * e + 2] = q.z * P.alpha_scale;
                    } else {                    // composite: src.a *= alpha_scale, src.rgb *= src.a (:130-131)
                        lut[4 * e + 0] = q.x * a; lut[4 * e + 1] = q.y * a; lut[4 * e + 2] = q.z * a;
                    }
                    lut[4 * e + 3] = a;
                }
            }
            __syncthreads();
        }
    }

    float drgb = 0.0f, dg = 0.0f, db = 0.0f, da = 0.0f;   // MODE 0/1: r == g == b bit for bit, only drgb is carried
    if (ngroups != 0u) {
        // (the packed format's base: 0 otherwise)
        const int base = PACK ? P.pk12_base : 0;
        const int cmin = P.min_val - base, cmax = P.max_val - base;
        const int lut_bias = MODE >= 2 ? FAST_TF_ENTRIES * 16 - cmin : -8 * cmin;
        uint32_t lut_entry0 = lds_offset_of(lut) + (uint32_t)lut_bias;
        asm volatile("" : "+v"(lut_entry0));                 // a VECTOR register: no SGPR operand in the sample loop's VALU
        // (the window's constants in VECTOR registers too: the table-less path has seven VALU operations per sample that read one)
        float wfmin = P.fmin, wfmax = P.fmax, wfden = P.fden, wrden = P.rden, walpha = P.alpha_scale;
        if (PACK && !BASEADD) { wfmin -= (float)base; wfmax -= (float)base; }      // exact (streamBaseFoldsIntoWindow)
        asm volatile("" : "+v"(wfmin), "+v"(wfmax), "+v"(wfden), "+v"(wrden), "+v"(walpha));
        // window + classification of one texel -> premultiplied colour and opacity (classify of vr_fast.hip:192-216, on the raw
        // voxel: the stream is no packed copy, there is no base to subtract; PACK: on voxel - base, against the shifted constants)
        auto classify = [&](uint32_t texel, float &c, float &cg, float &cb, float &a) {
            if (LUT) {
                int v = (int)texel;
                if (!NOCLAMP) v = med3_i32(v, cmin, cmax);             // clamp(texel, min_val, max_val), min <= max
                if (MODE >= 2) {
                    const uint32_t idx = reinterpret_cast<const uint8_t *>(lut)[(uint32_t)(v + lut_bias)];
                    const float4 q = reinterpret_cast<const float4 *>(lut)[idx];
                    c = q.x; cg = q.y; cb = q.z; a = q.w;
                } else {
                    uint32_t entry;
                    asm("v_lshl_add_u32 %0, %1, 3, %2" : "=v"(entry) : "v"(v), "v"(lut_entry0));
                    VR_LDS_AS const float *ca = reinterpret_cast<VR_LDS_AS const float *>((size_t)entry);      // (one ds_read_b64)
                    c = ca[0]; a = ca[1];
                }
            } else {
                float s = (float)texel;
                if (!NOCLAMP) s = fminf(fmaxf(s, wfmin), wfmax);   // operands are never NaN here
                s = div_cert(s - wfmin, wfden, wrden);
                a = s * walpha;
                c = s * a;
            }
        };
        // the hybrid's table sample: the entry of clamp(texel) -- the (c, a) the arithmetic above gives, computed by the same
        // operations when the table was built.  Only the read is issued here: the loop below asks for a group's entries one
        // group ahead of their use
        auto table_read = [&](uint32_t texel) -> stream_f32x2 {
            int v = (int)texel;
            if (!NOCLAMP) v = med3_i32(v, cmin, cmax);
            uint32_t entry;
            asm("v_lshl_add_u32 %0, %1, 3, %2" : "=v"(entry) : "v"(v), "v"(lut_entry0));
            return *reinterpret_cast<VR_LDS_AS const stream_f32x2 *>((size_t)entry);     // (one ds_read_b64: an entry is 8-byte aligned)
        };
        // which of a group's four samples go through the table: the same positions in every lane
        auto table_pos = [](int u) { return TSHARE == 4 || (TSHARE == 2 && (u & 1) != 0) || (TSHARE == 1 && u == 3); };
        // one sample onto the destination: front-to-back composite (VolumeRenderer.cs:132-133) or MIP's running maximum
        // (:165-168) -- accumulate of vr_fast.hip:334-345
        auto accumulate = [&](float c, float cg, float cb, float a) {
            if (MODE == 1) {
                if (da < a) da = a;
            } else if (MODE == 3) {
                if (da < a) { drgb = c; dg = cg; db = cb; da = a; }
            } else {
                const float om = 1.0f - da;
                drgb += c * om;
                if (MODE == 2) { dg += cg * om; db += cb * om; }
                da += a * om;
            }
        };
        using GroupT = typename std::conditional<PACK, stream_u32x3, typename std::conditional<sizeof(VoxelT) == 2, stream_u32x2, uint32_t>::type>::type;
        // (PACK: the block's bytes begin at off / 2 * 3, a lane's 12 bytes of a group at l * 12 of the group's 768)
        using SlotT = typename std::conditional<PACK, uint32_t, GroupT>::type;
        constexpr unsigned SLOTS = PACK ? 3u : 1u;           // of SlotT per lane per group
        const SlotT *sp = PACK ? reinterpret_cast<const SlotT *>(reinterpret_cast<const uint8_t *>(samples) + off / 2u * 3u) + lane * SLOTS
                               : reinterpret_cast<const SlotT *>(samples + off) + lane;
        // group g of this lane; past the block's last group the last one is read again (its samples are never composited):
        // the loop below is straight-line code with a fixed number of loads in flight
        auto load_group = [&](uint32_t g) -> GroupT {
            const SlotT *p = sp + (size_t)min(g, ngroups - 1u) * (64u * SLOTS);
            if constexpr (PACK) {                            // (three dword loads at one address: the compiler makes them one of 12 bytes)
                GroupT w;
                w.x = VR_STREAM_NT ? __builtin_nontemporal_load(p) : p[0];
                w.y = VR_STREAM_NT ? __builtin_nontemporal_load(p + 1) : p[1];
                w.z = VR_STREAM_NT ? __builtin_nontemporal_load(p + 2) : p[2];
                return w;
            } else {
                return VR_STREAM_NT ? __builtin_nontemporal_load(p) : *p;
            }
        };
        auto texel_of = [&](const GroupT &w, int u) -> uint32_t {
            if constexpr (PACK) return stream_unpack12(w.x, w.y, w.z, u) + (BASEADD ? (uint32_t)base : 0u);
            else if constexpr (sizeof(VoxelT) == 2) return u & 1 ? w[u >> 1] >> 16 : w[u >> 1] & 0xffffu;
            else return (w >> (8 * u)) & 0xffu;
        };
        bool alive = n > 0;
        // the G samples i0 .. i0 + G - 1.  alpha_scale in [0,1] (fast-path precondition) makes dest.a non-decreasing and <= 1,
        // so "dest.a < 0.95 before the LAST sample" proves the shader's per-sample test `dest.a >= 0.95 -> break`
        // (VolumeRenderer.cs:118) passed for the whole group; the group in which a ray ends -- by that test or at its own n --
        // runs the literal per-sample tests, and its padded slots are never composited.  u0: the first of the four inside the
        // load's group (PACK: a group of 8 is consumed as two groups of four, u0 = 0 and 4)
        // te (TSHARE): the table entries of the four, read ahead (table_read), valid at the table positions
        auto consume = [&](const GroupT &w, int i0, int u0, const stream_f32x2 *te) {
            if (!alive) return;
            float c[STREAM_G], cg[STREAM_G], cb[STREAM_G], a[STREAM_G];
            if constexpr (TSHARE > 0) {
                // the arithmetic samples first: they cover what is left of the table reads' latency
#pragma unroll
                for (int u = 0; u < (int)STREAM_G; u++) { cg[u] = 0.0f; cb[u] = 0.0f; if (!table_pos(u)) classify(texel_of(w, u0 + u), c[u], cg[u], cb[u], a[u]); }
#pragma unroll
                for (int u = 0; u < (int)STREAM_G; u++) {
                    if (table_pos(u)) { c[u] = te[u].x; a[u] = te[u].y; }
                }
            } else {
#pragma unroll
                for (int u = 0; u < (int)STREAM_G; u++) { cg[u] = 0.0f; cb[u] = 0.0f; classify(texel_of(w, u0 + u), c[u], cg[u], cb[u], a[u]); }
            }
            const float drgb0 = drgb, dg0 = dg, db0 = db, da0 = da;
            float da_last = 0.0f;
#pragma unroll
            for (int u = 0; u < (int)STREAM_G; u++) {
                if (u == (int)STREAM_G - 1) da_last = da;
                accumulate(c[u], cg[u], cb[u], a[u]);
            }
            if (i0 + (int)STREAM_G <= n && da_last < 0.95f) return;
            drgb = drgb0; dg = dg0; db = db0; da = da0;
#pragma unroll
            for (int u = 0; u < (int)STREAM_G; u++) {
                if (i0 + u >= n || da >= 0.95f) { alive = false; return; }
                accumulate(c[u], cg[u], cb[u], a[u]);
            }
        };
        constexpr int K = PACK ? VR_STREAM12_DEPTH : VR_STREAM_DEPTH;
        GroupT cur[K], nxt[K];
#pragma unroll
        for (int k = 0; k < K; k++) cur[k] = load_group((uint32_t)k);
        for (uint32_t g0 = 0; g0 < ngroups; g0 += (uint32_t)K) {
#pragma unroll
            for (int k = 0; k < K; k++) nxt[k] = load_group(g0 + (uint32_t)(K + k));
            if constexpr (TSHARE > 0) {
                // a loaded group's table entries are asked for while the group before it is composited, by every lane (a lane
                // that has ended reads entries of its own slots: values of the volume, or the padding's), and waited for in
                // the order they were asked
                stream_f32x2 te[2][G];
                auto table_group = [&](const GroupT &w, stream_f32x2 *e) {
#pragma unroll
                    for (int u = 0; u < (int)G; u++) if (table_pos(u % (int)STREAM_G)) e[u] = table_read(texel_of(w, u));
                };
                table_group(cur[0], te[0]);
#pragma unroll
                for (int k = 0; k < K; k++) {
                    if (k + 1 < K) table_group(cur[k + 1], te[(k + 1) & 1]);
                    consume(cur[k], (int)((g0 + (uint32_t)k) * G), 0, te[k & 1]);
                    if (PACK) consume(cur[k], (int)((g0 + (uint32_t)k) * G + STREAM_G), (int)STREAM_G, te[k & 1] + STREAM_G);
                }
            } else {
#pragma unroll
                for (int k = 0; k < K; k++) {
                    consume(cur[k], (int)((g0 + (uint32_t)k) * G), 0, nullptr);
                    if (PACK) consume(cur[k], (int)((g0 + (uint32_t)k) * G + STREAM_G), (int)STREAM_G, nullptr);
                }
            }
#pragma unroll
            for (int k = 0; k < K; k++) cur[k] = nxt[k];
            if (__builtin_amdgcn_ballot_w64(alive) == 0ull) break;      // no lane of the wavefront is alive
        }
    }
    if (!in_image) return;
    const size_t pix = (size_t)(P.fb_compact ? ly : py) * (size_t)P.img_w + (size_t)px;
    if (MODE >= 2) store_pixel(P, fb, pix, drgb, dg, db, da);
    else if (MODE == 1) store_pixel(P, fb, pix, da, da, da, da);
    else store_pixel(P, fb, pix, drgb, drgb, drgb, da);
}

template <typename VoxelT, int MODE, bool PACK>
static hipError_t launch_replay_mode(const FrameParams &P, const LaunchConfig &L, const float4 *tf, float4 *fb, const RayStreamView &S, hipStream_t st)
{
    const StreamGrid g = streamGrid(P.img_w, launch_local_rows(P));
    const dim3 grid(L.tile_table_blocks), block(512);
    // (a table-less instance's grid: 512 / VR_STREAM_WG workgroups per tile, their product kept inside a grid's 2^31 - 1)
    constexpr unsigned SPLIT = 512u / (unsigned)VR_STREAM_WG;
    if (L.tile_table_blocks > 0x7fffffffu / SPLIT) return hipErrorInvalidValue;
    const dim3 grid_nolut(L.tile_table_blocks * SPLIT), block_nolut((unsigned)VR_STREAM_WG);
    // Without S.table the grey ramp is classified ARITHMETICALLY, whatever the window: a table look-up asked for when the sample
    // is composited (one read per sample at a data-dependent address, what the gather kernels and the LUT instances do) is
    // what this kernel would wait for -- cfg3 0.246 ms with it, 0.226 without (docs/lab-notebook.md) -- and the table's
    // entries are these same operations, so the bits are the same.  Tables remain for the transfer function (MODE >= 2) and
    // its grey fold.
    const bool lut = MODE >= 2 ? L.use_lut != 0 : P.tf_grey != 0;
    // The hybrid (S.table; streamTableEligible): VR_STREAM_TSHARE of every four samples through the table, every read asked for
    // one loaded group ahead of its use, in workgroups of VR_STREAM_TWG threads that share one table.  The table samples' bits
    // are the arithmetic samples' (the entries are those operations), so the choice never shows in a frame.
    static_assert(kStreamTableMax == FAST_LUT_MAX, "vr_stream.h: kStreamTableMax");
    const bool hybrid = MODE < 2 && S.table != 0 && streamTableEligible(P, L, S);
    constexpr unsigned TSPLIT = 512u / (unsigned)VR_STREAM_TWG;
    const dim3 grid_t(L.tile_table_blocks * TSPLIT), block_t((unsigned)VR_STREAM_TWG);
    if constexpr (PACK) {
        // the stream's own base travels in the frame's parameters (pk12_base is otherwise the packed volume copy's, which the
        // replay never reads); a window the shifted constants cannot hold exactly takes the integer add (BASEADD)
        FrameParams Q = P;
        Q.pk12_base = S.base;
        const bool shift = streamBaseFoldsIntoWindow(P.min_val, P.max_val, S.base);
#define VR_REPLAY12(LT, NC, BA)                                                                                                   \
    hipLaunchKernelGGL((raymarch_stream_kernel<VoxelT, MODE, LT, NC, true, BA>), LT ? grid : grid_nolut, LT ? block : block_nolut, 0, st, Q, tf, fb, \
                       (const VoxelT *)S.samples, S.counts, S.offsets, g.blocks_x, L.tile_table)
#define VR_REPLAY12_T1(TS) hipLaunchKernelGGL((raymarch_stream_kernel<VoxelT, MODE, false, true, true, false, TS>), grid_t, block_t, 0, st, Q, tf, fb, \
                                              (const VoxelT *)S.samples, S.counts, S.offsets, g.blocks_x, L.tile_table)
#define VR_REPLAY12_T0(TS) hipLaunchKernelGGL((raymarch_stream_kernel<VoxelT, MODE, false, false, true, false, TS>), grid_t, block_t, 0, st, Q, tf, fb, \
                                              (const VoxelT *)S.samples, S.counts, S.offsets, g.blocks_x, L.tile_table)
        if constexpr (MODE == 0) {
            if (lut) VR_REPLAY12(true, false, false);
            else if (hybrid) { if (L.lut_noclamp != 0) VR_REPLAY12_T1(VR_STREAM_TSHARE); else VR_REPLAY12_T0(VR_STREAM_TSHARE); }
            else if (L.lut_noclamp != 0) { if (shift) VR_REPLAY12(false, true, false); else VR_REPLAY12(false, true, true); }
            else { if (shift) VR_REPLAY12(false, false, false); else VR_REPLAY12(false, false, true); }
        } else if constexpr (MODE == 1) {
            if (hybrid) VR_REPLAY12_T0(VR_STREAM_TSHARE);
            else if (shift) VR_REPLAY12(false, false, false); else VR_REPLAY12(false, false, true);
        } else {
            if (!lut) return hipErrorInvalidValue;
            VR_REPLAY12(true, false, false);
        }
#undef VR_REPLAY12_T0
#undef VR_REPLAY12_T1
#undef VR_REPLAY12
        return hipGetLastError();
    } else {
#define VR_REPLAY(LT, NC)                                                                                                        \
    hipLaunchKernelGGL((raymarch_stream_kernel<VoxelT, MODE, LT, NC>), LT ? grid : grid_nolut, LT ? block : block_nolut, 0, st, P, tf, fb, (const VoxelT *)S.samples, \
                       S.counts, S.offsets, g.blocks_x, L.tile_table)
#define VR_REPLAY_T1(TS) hipLaunchKernelGGL((raymarch_stream_kernel<VoxelT, MODE, false, true, false, false, TS>), grid_t, block_t, 0, st, P, tf, fb, \
                                            (const VoxelT *)S.samples, S.counts, S.offsets, g.blocks_x, L.tile_table)
#define VR_REPLAY_T0(TS) hipLaunchKernelGGL((raymarch_stream_kernel<VoxelT, MODE, false, false, false, false, TS>), grid_t, block_t, 0, st, P, tf, fb, \
                                            (const VoxelT *)S.samples, S.counts, S.offsets, g.blocks_x, L.tile_table)
    if constexpr (MODE == 0) {
        if (lut) VR_REPLAY(true, false);
        else if (hybrid) { if (L.lut_noclamp != 0) VR_REPLAY_T1(VR_STREAM_TSHARE); else VR_REPLAY_T0(VR_STREAM_TSHARE); }
        else if (L.lut_noclamp != 0) VR_REPLAY(false, true);            // the data's exact range lies inside the window: clamp() is the identity
        else VR_REPLAY(false, false);
    } else if constexpr (MODE == 1) {
        if (hybrid) VR_REPLAY_T0(VR_STREAM_TSHARE); else VR_REPLAY(false, false);
    } else {
        if (!lut) return hipErrorInvalidValue;               // (fast_path_eligible: a transfer function needs the table)
        VR_REPLAY(true, false);
    }
#undef VR_REPLAY_T0
#undef VR_REPLAY_T1
#undef VR_REPLAY
    return hipGetLastError();
    }
}

// the mode as dispatch_fast2 picks it (vr_kernels.hip)
template <typename VoxelT, bool PACK = false>
static hipError_t launch_replay_type(const FrameParams &P, const LaunchConfig &L, const float4 *tf, float4 *fb, const RayStreamView &S, hipStream_t st)
{
    if (L.mip && P.tf_len > 1) return launch_replay_mode<VoxelT, 3, PACK>(P, L, tf, fb, S, st);
    if (L.mip) return launch_replay_mode<VoxelT, 1, PACK>(P, L, tf, fb, S, st);
    if (P.tf_len > 1 && P.tf_grey == 0) return launch_replay_mode<VoxelT, 2, PACK>(P, L, tf, fb, S, st);
    return launch_replay_mode<VoxelT, 0, PACK>(P, L, tf, fb, S, st);
}

#if VR_STREAM_TU == 2
// the packed format's instances (16-bit volumes)
hipError_t launch_stream_record_p12(const FrameParams &P, const LaunchConfig &L, const void *vol, uint16_t *counts, const uint64_t *offsets,
                                    void *samples, int base, hipStream_t st)
{
    FrameParams Q = P;
    Q.pk12_base = base;
    return launch_record_type<uint16_t, true>(Q, L, vol, counts, nullptr, offsets, samples, STREAM12_G, st);
}
hipError_t launch_raymarch_stream_p12(const FrameParams &P, const LaunchConfig &L, const float4 *tf, float4 *fb, const RayStreamView &S, hipStream_t st)
{
    return launch_replay_type<uint16_t, true>(P, L, tf, fb, S, st);
}
#endif

#if VR_STREAM_TU == 1
hipError_t launch_stream_record_u16(const FrameParams &P, const LaunchConfig &L, const void *vol, uint16_t *counts, uint32_t *block_elems,
                                    const uint64_t *offsets, void *samples, hipStream_t st)
{
    return launch_record_type<uint16_t>(P, L, vol, counts, block_elems, offsets, samples, STREAM_G, st);
}
hipError_t launch_raymarch_stream_u16(const FrameParams &P, const LaunchConfig &L, const float4 *tf, float4 *fb, const RayStreamView &S, hipStream_t st)
{
    return launch_replay_type<uint16_t>(P, L, tf, fb, S, st);
}
#endif

#if VR_STREAM_TU == 0
hipError_t launch_stream_record_u16(const FrameParams &P, const LaunchConfig &L, const void *vol, uint16_t *counts, uint32_t *block_elems,
                                    const uint64_t *offsets, void *samples, hipStream_t st);
hipError_t launch_raymarch_stream_u16(const FrameParams &P, const LaunchConfig &L, const float4 *tf, float4 *fb, const RayStreamView &S, hipStream_t st);
hipError_t launch_stream_record_p12(const FrameParams &P, const LaunchConfig &L, const void *vol, uint16_t *counts, const uint64_t *offsets,
                                    void *samples, int base, hipStream_t st);
hipError_t launch_raymarch_stream_p12(const FrameParams &P, const LaunchConfig &L, const float4 *tf, float4 *fb, const RayStreamView &S, hipStream_t st);

// exclusive scan of the blocks' padded lengths: one workgroup, every thread a contiguous run of blocks (a one-off of at most a
// few hundred thousand entries)
__global__ __launch_bounds__(1024) void stream_scan_kernel(const uint32_t *__restrict__ block_elems, uint64_t *__restrict__ offsets, const unsigned blocks)
{
    __shared__ uint64_t part[1024];
    const unsigned per = (blocks + 1023u) / 1024u;
    const unsigned b0 = min(threadIdx.x * per, blocks), b1 = min(b0 + per, blocks);
    uint64_t sum = 0;
    for (unsigned b = b0; b < b1; b++) sum += block_elems[b];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (unsigned d = 1; d < 1024u; d <<= 1) {               // inclusive Hillis-Steele scan of the 1024 partial sums
        const uint64_t add = threadIdx.x >= d ? part[threadIdx.x - d] : 0ull;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    uint64_t run = part[threadIdx.x] - sum;
    for (unsigned b = b0; b < b1; b++) { offsets[b] = run; run += block_elems[b]; }
    if (threadIdx.x == 1023u) offsets[blocks] = part[1023];
}

hipError_t launch_stream_scan(const uint32_t *block_elems, uint64_t *offsets, unsigned blocks, hipStream_t st)
{
    hipLaunchKernelGGL(stream_scan_kernel, dim3(1), dim3(1024), 0, st, block_elems, offsets, blocks);
    return hipGetLastError();
}

// block lengths counted for a smaller group size, rounded up to whole groups of `group` (a multiple of it): ceil_8(ceil_4(n)) ==
// ceil_8(n), so the count pass need not run again when the format is chosen from the unpacked size
__global__ __launch_bounds__(256) void stream_regroup_kernel(uint32_t *__restrict__ block_elems, const unsigned blocks, const unsigned group)
{
    const unsigned b = blockIdx.x * 256u + threadIdx.x;
    if (b >= blocks) return;
    block_elems[b] = ((block_elems[b] / 64u + group - 1u) / group) * (64u * group);
}

hipError_t launch_stream_regroup(uint32_t *block_elems, unsigned blocks, unsigned group, hipStream_t st)
{
    if (blocks == 0u || group == 0u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(stream_regroup_kernel, dim3((blocks + 255u) / 256u), dim3(256), 0, st, block_elems, blocks, group);
    return hipGetLastError();
}

hipError_t launch_stream_count(const FrameParams &P, const LaunchConfig &L, uint16_t *counts, uint32_t *block_elems, unsigned group, hipStream_t st)
{
    if (group == 0u) return hipErrorInvalidValue;
    // (the count pass reads no voxel: the 8-bit instance serves both types)
    return launch_record_type<uint8_t>(P, L, nullptr, counts, block_elems, nullptr, nullptr, group, st);
}

hipError_t launch_stream_record(const FrameParams &P, const LaunchConfig &L, const void *vol, const uint16_t *counts,
                                const uint64_t *offsets, void *samples, StreamFormat format, int base, hipStream_t st)
{
    if (samples == nullptr) return hipErrorInvalidValue;
    uint16_t *c = const_cast<uint16_t *>(counts);            // (the record pass only reads them)
    if (format == kStreamPack12)
        return L.bytes_per_voxel == 2 ? launch_stream_record_p12(P, L, vol, c, offsets, samples, base, st) : hipErrorInvalidValue;
    return L.bytes_per_voxel == 1 ? launch_record_type<uint8_t>(P, L, vol, c, nullptr, offsets, samples, STREAM_G, st)
                                  : launch_stream_record_u16(P, L, vol, c, nullptr, offsets, samples, st);
}

hipError_t launch_raymarch_stream(const FrameParams &P, const LaunchConfig &L, const float4 *tf, float4 *fb, const RayStreamView &S,
                                  hipStream_t st, const char **kernel_name)
{
    if (launch_local_rows(P) <= 0 || P.img_w <= 0) return hipSuccess;
    if (L.tile_table == nullptr || S.samples == nullptr) return hipErrorInvalidValue;
    if (S.format == kStreamPack12) {
        if (L.bytes_per_voxel != 2) return hipErrorInvalidValue;
        if (kernel_name) *kernel_name = "raymarch_stream12_kernel";
        return launch_raymarch_stream_p12(P, L, tf, fb, S, st);
    }
    if (kernel_name) *kernel_name = "raymarch_stream_kernel";
    return L.bytes_per_voxel == 1 ? launch_replay_type<uint8_t>(P, L, tf, fb, S, st) : launch_raymarch_stream_u16(P, L, tf, fb, S, st);
}
#endif

VR_CODE_UNIT(stream, VR_STREAM_TU, "sample stream", WARM_LOAD_SHADER)

}  // namespace vr
