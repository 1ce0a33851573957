// vr_smooth.hip -- separable Gaussian smoothing of the resident volume (vr_smooth_volume).  The definition, operation by
// operation, is in include/vr_core.h and DESIGN.md section 1.4; tests/smooth_ref/smooth_ref.c restates it on the CPU and
// tests/test_smoothing_gpu.py holds these kernels to it bit for bit.
//
// Its own translation units (VR_SMOOTH_TU = 0: 8-bit volumes, 1: 16-bit volumes), like vr_shade.hip.
// Arithmetic contract: per output and pass acc = 0.0f, then acc = acc + w_t * in[clamp(i + t)] for t = -r .. r in increasing
// order, the product rounded, then the sum (-ffp-contract=off: nothing becomes an fma).  The kernels run that recurrence over
// a weight vector padded with zeros on both sides, so that a lane's four outputs share every LDS read: a padding term is
// w = 0 times a finite value >= 0, i.e. +0, and acc + (+0) == acc bit for bit (acc is never -0: it starts at +0 and only adds
// products of non-negative numbers).  The padded terms come before the first and after the last real one, so the order of the
// real ones is the definition's.
//
// Shape: three global passes (x, then y, then z; an axis with sigma 0 has none), fp32 planes between them, every pass one
// kernel of 256-thread workgroups that stage their input in LDS once and compute four outputs along x per lane (one vector
// store each).
//   x: a workgroup owns 128 x 4 x 4 outputs (whole bricks of a bricked volume); it stages the 16 rows with their halo.
//   y, z: a workgroup owns 64 x 4 outputs across the axis and MARCHES along it, 16 rows per step, through a ring of rows in LDS:
//      a row is read from memory once per workgroup, whatever the radius (the halo is re-read only where two segments meet).
// Every load clamps its coordinates into the volume (that IS the edge rule) and, for fp32 planes, into the planes the buffer
// holds; every store is guarded by the volume and the pass's plane range.  Index arithmetic is 64-bit throughout.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "vr_code_unit.h"
#include "vr_frame.h"
#include "vr_smooth.h"

#ifndef VR_SMOOTH_TU
#error "VR_SMOOTH_TU: the unit number comes from the build"
#endif

namespace vr {

namespace {

constexpr int kPad = 3;                                  // zeros in front of the weights: a lane's outputs m = 0 .. 3 read w[p - m]
constexpr int kPaddedWeights = 2 * kSmoothMaxRadius + 1 + 2 * kPad + 1;   // 56: indices up to 4 * 13 + 2 (x pass), 2r + 6 (y, z)

struct SmoothArgs {
    const void *in;
    void *out;
    uint32_t nx, ny, nz, bnx, bny;
    int32_t layout;
    int32_t in_z0, in_planes, out_z0, out_planes;
    int32_t z_begin, z_end;
    int32_t r;
    int32_t seg;                                         // y, z passes: outputs along the axis per workgroup (a multiple of 16)
    float wp[kPaddedWeights];                            // wp[kPad + t] = w_t, t = 0 .. 2r; zeros elsewhere
};

__device__ __forceinline__ uint64_t voxel_index(const SmoothArgs &A, uint32_t i, uint32_t j, uint32_t k)
{
    if (A.layout == 0) return (uint64_t)i + (uint64_t)A.nx * ((uint64_t)j + (uint64_t)A.ny * (uint64_t)k);
    const uint64_t brick = (uint64_t)(i >> BRICK_LX) + (uint64_t)A.bnx * ((uint64_t)(j >> BRICK_LY) + (uint64_t)A.bny * (uint64_t)(k >> BRICK_LZ));
    return brick * 64u + ((i & (BRICK_X - 1u)) | ((j & (BRICK_Y - 1u)) << BRICK_LX) | ((k & (BRICK_Z - 1u)) << (BRICK_LX + BRICK_LY)));
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// in[x, y, z] as fp32; the coordinates are inside the volume
template <typename InT>
__device__ __forceinline__ float load_in(const SmoothArgs &A, int x, int y, int z)
{
    if constexpr (sizeof(InT) == 4) {
        const int p = clampi(z - A.in_z0, 0, A.in_planes - 1);          // (the host keeps every plane a pass reads in the buffer)
        return static_cast<const float *>(A.in)[(uint64_t)x + (uint64_t)A.nx * ((uint64_t)y + (uint64_t)A.ny * (uint64_t)p)];
    } else {
        return (float)static_cast<const InT *>(A.in)[voxel_index(A, (uint32_t)x, (uint32_t)y, (uint32_t)z)];
    }
}

typedef float float4v __attribute__((ext_vector_type(4)));
typedef uint8_t uchar4v __attribute__((ext_vector_type(4)));
typedef uint16_t ushort4v __attribute__((ext_vector_type(4)));

// the last pass's rounding: half to even, then the clamp to the voxel type
template <typename OutT>
__device__ __forceinline__ OutT to_voxel(float v)
{
    const float hi = sizeof(OutT) == 1 ? 255.0f : 65535.0f;
    const float q = fminf(fmaxf(rintf(v), 0.0f), hi);
    return (OutT)(uint32_t)q;
}

// four outputs at (x .. x + 3, y, z); x is a multiple of 4 and inside the volume, y and z are inside the pass's range
template <typename OutT>
__device__ __forceinline__ void store_quad(const SmoothArgs &A, int x, int y, int z, const float v[4])
{
    const int n = (int)A.nx - x < 4 ? (int)A.nx - x : 4;
    if constexpr (sizeof(OutT) == 4) {
        const int p = z - A.out_z0;
        if (p < 0 || p >= A.out_planes) return;
        float *o = static_cast<float *>(A.out) + ((uint64_t)x + (uint64_t)A.nx * ((uint64_t)y + (uint64_t)A.ny * (uint64_t)p));
        if (n == 4 && ((uintptr_t)o & 15u) == 0) {
            *reinterpret_cast<float4v *>(o) = float4v{v[0], v[1], v[2], v[3]};
        } else {
            for (int m = 0; m < n; m++) o[m] = v[m];
        }
    } else {
        // a quad starts a brick row (BRICK_X == 4) or, in the linear layout, lies in one row of the volume: contiguous either way
        OutT *o = static_cast<OutT *>(A.out) + voxel_index(A, (uint32_t)x, (uint32_t)y, (uint32_t)z);
        const OutT q0 = to_voxel<OutT>(v[0]), q1 = to_voxel<OutT>(v[1]), q2 = to_voxel<OutT>(v[2]), q3 = to_voxel<OutT>(v[3]);
        if (n == 4 && ((uintptr_t)o & (4 * sizeof(OutT) - 1)) == 0) {
            if constexpr (sizeof(OutT) == 1) *reinterpret_cast<uchar4v *>(o) = uchar4v{q0, q1, q2, q3};
            else *reinterpret_cast<ushort4v *>(o) = ushort4v{q0, q1, q2, q3};
        } else {
            const OutT q[4] = {q0, q1, q2, q3};
            for (int m = 0; m < n; m++) o[m] = q[m];
        }
    }
}
static_assert(BRICK_X == 4, "store_quad writes one brick row per quad");

// ------------------------------------------------------------------ the pass along x
constexpr int kXTile = 128, kXRows = 16, kXStride = 180;   // 124 + 4 * 13 floats staged per row at the largest radius; rows 16-byte aligned

template <typename VoxelT, typename InT, typename OutT>
__global__ __launch_bounds__(256) void smooth_x_kernel(const SmoothArgs A)
{
    __shared__ __attribute__((aligned(16))) float s[kXRows * kXStride];
    const int tiles_x = ((int)A.nx + kXTile - 1) / kXTile;
    const int x0 = (int)(blockIdx.x % (uint32_t)tiles_x) * kXTile, y0 = (int)(blockIdx.x / (uint32_t)tiles_x) * 4;
    const int z0 = A.z_begin + (int)blockIdx.y * 4;
    const int nch = (2 * A.r + 7) / 4;                   // float4 chunks a lane reads: 4 outputs + 2r neighbours, rounded up
    const int width = kXTile - 4 + 4 * nch;              // floats staged per row (<= 176)
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    for (int row = wave; row < kXRows; row += 4) {
        const int y = min(y0 + (row & 3), (int)A.ny - 1), z = min(z0 + (row >> 2), A.z_end - 1);
        for (int p = lane; p < width; p += 64)
            s[row * kXStride + p] = load_in<InT>(A, clampi(x0 - A.r + p, 0, (int)A.nx - 1), y, z);
    }
    __syncthreads();
    const int xq = (int)threadIdx.x & 31;
    for (int h = 0; h < 2; h++) {
        const int row = ((int)threadIdx.x >> 5) + 8 * h;
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int c = 0; c < nch; c++) {
            const float4v v = *reinterpret_cast<const float4v *>(&s[row * kXStride + 4 * xq + 4 * c]);
#pragma unroll
            for (int e = 0; e < 4; e++)
#pragma unroll
                for (int m = 0; m < 4; m++) acc[m] = acc[m] + A.wp[4 * c + e - m + kPad] * v[e];
        }
        const int x = x0 + 4 * xq, y = y0 + (row & 3), z = z0 + (row >> 2);
        if (x < (int)A.nx && y < (int)A.ny && z < A.z_end) store_quad<OutT>(A, x, y, z, acc);
    }
}

// ------------------------------------------------------------------ the passes along y and z
// AXIS 1: a = y, b = z (the pass's planes).  AXIS 2: a = z (the pass's planes), b = y.
// RING: rows the LDS ring holds, 32 (32 KiB, five workgroups per CU) where a step's 16 rows and both halos fit, i.e. r <= 8,
// else 64 (64 KiB, two per CU).  VoxelT only names the instance: the fp32 -> fp32 pass exists once per translation unit, and
// the two units' instances must be different symbols.
template <typename VoxelT, typename InT, typename OutT, int AXIS, int RING>
__global__ __launch_bounds__(256) void smooth_col_kernel(const SmoothArgs A)
{
    __shared__ __attribute__((aligned(16))) float ring[RING * 4 * 64];
    const int tiles_x = ((int)A.nx + 63) / 64;
    const int x0 = (int)(blockIdx.x % (uint32_t)tiles_x) * 64;
    const int b_begin = AXIS == 1 ? A.z_begin : 0, b_end = AXIS == 1 ? A.z_end : (int)A.ny;
    const int a_begin = AXIS == 1 ? 0 : A.z_begin, a_end = AXIS == 1 ? (int)A.ny : A.z_end;
    const int a_dim = AXIS == 1 ? (int)A.ny : (int)A.nz;
    const int b0 = b_begin + (int)(blockIdx.x / (uint32_t)tiles_x) * 4;
    const int seg0 = a_begin + (int)blockIdx.y * A.seg, seg1 = min(seg0 + A.seg, a_end);
    const int r = A.r;
    // staging: row `ar` of the ring's numbering is a = seg0 - r + ar; each thread one element of a row
    const int lx = min(x0 + ((int)threadIdx.x & 63), (int)A.nx - 1), lb = min(b0 + ((int)threadIdx.x >> 6), b_end - 1);
    auto stage = [&](int ar) {
        const int a = clampi(seg0 - r + ar, 0, a_dim - 1);
        ring[(ar & (RING - 1)) * 256 + (int)threadIdx.x] = AXIS == 1 ? load_in<InT>(A, lx, a, lb) : load_in<InT>(A, lx, lb, a);
    };
    for (int ar = 0; ar < 2 * r; ar++) stage(ar);
    const int xq = (int)threadIdx.x & 15, bb = ((int)threadIdx.x >> 4) & 3, aq = (int)threadIdx.x >> 6;
    for (int a0 = seg0; a0 < seg1; a0 += 16) {
        const int base = a0 - seg0;
#pragma unroll
        for (int i = 0; i < 16; i++) stage(base + 2 * r + i);
        __syncthreads();
        float acc[4][4];
#pragma unroll
        for (int m = 0; m < 4; m++)
#pragma unroll
            for (int e = 0; e < 4; e++) acc[m][e] = 0.0f;
        for (int p = 0; p < 2 * r + 4; p++) {
            const float4v v = *reinterpret_cast<const float4v *>(&ring[((base + 4 * aq + p) & (RING - 1)) * 256 + bb * 64 + 4 * xq]);
#pragma unroll
            for (int m = 0; m < 4; m++) {
                const float w = A.wp[p - m + kPad];
#pragma unroll
                for (int e = 0; e < 4; e++) acc[m][e] = acc[m][e] + w * v[e];
            }
        }
        const int x = x0 + 4 * xq, b = b0 + bb;
        if (x < (int)A.nx && b < b_end) {
#pragma unroll
            for (int m = 0; m < 4; m++) {
                const int a = a0 + 4 * aq + m;
                if (a < seg1) {
                    if (AXIS == 1) store_quad<OutT>(A, x, a, b, acc[m]);
                    else store_quad<OutT>(A, x, b, a, acc[m]);
                }
            }
        }
        __syncthreads();                                 // the next step's rows overwrite the oldest ones
    }
}

template <typename VoxelT, typename InT, typename OutT>
hipError_t launch_x(const SmoothArgs &A, hipStream_t st)
{
    const uint64_t tiles = (uint64_t)((A.nx + kXTile - 1) / kXTile) * (uint64_t)((A.ny + 3) / 4);
    const uint32_t tz = (uint32_t)(A.z_end - A.z_begin + 3) / 4;
    if (tiles >= (1ull << 31) || tz > 65535u) return hipErrorInvalidValue;
    hipLaunchKernelGGL((smooth_x_kernel<VoxelT, InT, OutT>), dim3((uint32_t)tiles, tz), dim3(256), 0, st, A);
    return hipGetLastError();
}

template <typename VoxelT, typename InT, typename OutT, int AXIS>
hipError_t launch_col(SmoothArgs A, hipStream_t st)
{
    const int nb = AXIS == 1 ? A.z_end - A.z_begin : (int)A.ny, na = AXIS == 1 ? (int)A.ny : A.z_end - A.z_begin;
    const uint64_t tiles = (uint64_t)((A.nx + 63) / 64) * (uint64_t)((nb + 3) / 4);
    // One workgroup per column where the columns alone give 2048 workgroups (eight per CU, the grid-stride guideline's cap);
    // else the column is halved into segments, each a multiple of 16 outputs and not below 48 (a segment re-reads 2r halo
    // rows: shorter ones would read more halo than data at the larger radii).  Neither constant has been tuned by measurement.
    int seg = (na + 15) / 16 * 16;
    while (seg > 64 && tiles * (uint64_t)((na + seg - 1) / seg) < 2048) seg = (seg / 2 + 15) / 16 * 16;
    A.seg = seg;
    const uint32_t segs = (uint32_t)((na + seg - 1) / seg);
    if (tiles >= (1ull << 31) || segs > 65535u) return hipErrorInvalidValue;
    if (16 + 2 * A.r <= 32) hipLaunchKernelGGL((smooth_col_kernel<VoxelT, InT, OutT, AXIS, 32>), dim3((uint32_t)tiles, segs), dim3(256), 0, st, A);
    else hipLaunchKernelGGL((smooth_col_kernel<VoxelT, InT, OutT, AXIS, 64>), dim3((uint32_t)tiles, segs), dim3(256), 0, st, A);
    return hipGetLastError();
}
static_assert(16 + 2 * kSmoothMaxRadius <= 64, "the ring holds a step's 16 rows and both halos");

template <typename VoxelT>
hipError_t launch_smooth_type(const SmoothPass &S, hipStream_t st)
{
    SmoothArgs A = {};
    A.in = S.in; A.out = S.out;
    A.nx = (uint32_t)S.nx; A.ny = (uint32_t)S.ny; A.nz = (uint32_t)S.nz;
    A.bnx = (uint32_t)((S.nx + BRICK_X - 1) / BRICK_X); A.bny = (uint32_t)((S.ny + BRICK_Y - 1) / BRICK_Y);
    A.layout = S.layout;
    A.in_z0 = S.in_z0; A.in_planes = S.in_planes; A.out_z0 = S.out_z0; A.out_planes = S.out_planes;
    A.z_begin = S.z_begin; A.z_end = S.z_end;
    A.r = S.radius;
    for (int t = 0; t <= 2 * S.radius; t++) A.wp[kPad + t] = S.weights[t];
    const int io = (S.in_float ? 2 : 0) | (S.out_float ? 1 : 0);
    if (S.axis == 0) {
        if (io == 1) return launch_x<VoxelT, VoxelT, float>(A, st);
        if (io == 0) return launch_x<VoxelT, VoxelT, VoxelT>(A, st);
    } else if (S.axis == 1) {
        if (io == 0) return launch_col<VoxelT, VoxelT, VoxelT, 1>(A, st);
        if (io == 1) return launch_col<VoxelT, VoxelT, float, 1>(A, st);
        if (io == 2) return launch_col<VoxelT, float, VoxelT, 1>(A, st);
        return launch_col<VoxelT, float, float, 1>(A, st);
    } else {
        if (io == 0) return launch_col<VoxelT, VoxelT, VoxelT, 2>(A, st);
        if (io == 2) return launch_col<VoxelT, float, VoxelT, 2>(A, st);
    }
    return hipErrorInvalidValue;                         // x is never fed fp32 planes, z never writes them (the order is x, y, z)
}

}  // namespace

VR_CODE_UNIT(smooth, VR_SMOOTH_TU, "smoothing", WARM_LOAD_SHADER)

#if VR_SMOOTH_TU == 1
hipError_t launch_smooth_u16(const SmoothPass &S, hipStream_t st) { return launch_smooth_type<uint16_t>(S, st); }
#else
// the unit of 8-bit volumes also carries the entry points
hipError_t launch_smooth_u8(const SmoothPass &S, hipStream_t st) { return launch_smooth_type<uint8_t>(S, st); }
hipError_t launch_smooth_u16(const SmoothPass &S, hipStream_t st);

bool smooth_weights(float sigma, float *w, int capacity, int *radius)
{
    if (!(sigma > 0.0f) || !(sigma <= kSmoothMaxSigma) || !w) return false;
    const double s = (double)sigma;
    int r = (int)std::ceil(3.0 * s);
    if (r > kSmoothMaxRadius) r = kSmoothMaxRadius;
    if (capacity < 2 * r + 1) return false;
    double g[2 * kSmoothMaxRadius + 1], sum = 0.0;
    for (int t = -r; t <= r; t++) {
        g[t + r] = std::exp(-(double)(t * t) / (2.0 * s * s));
        sum += g[t + r];
    }
    for (int t = 0; t <= 2 * r; t++) w[t] = (float)(g[t] / sum);
    if (radius) *radius = r;
    return true;
}

hipError_t launch_smooth_pass(const SmoothPass &S, hipStream_t st)
{
    if (!S.in || !S.out || !S.weights || S.nx <= 0 || S.ny <= 0 || S.nz <= 0 || S.radius < 1 || S.radius > kSmoothMaxRadius ||
        S.axis < 0 || S.axis > 2 || S.z_begin < 0 || S.z_end > S.nz || (S.layout != 0 && S.layout != 1))
        return hipErrorInvalidValue;
    if (S.z_begin >= S.z_end) return hipSuccess;
    // every plane the pass reads or writes lies in its fp32 buffer
    const int lo = S.axis == 2 ? (S.z_begin - S.radius > 0 ? S.z_begin - S.radius : 0) : S.z_begin;
    const int hi = S.axis == 2 ? (S.z_end + S.radius < S.nz ? S.z_end + S.radius : S.nz) : S.z_end;
    if (S.in_float && (S.in_planes < 1 || lo < S.in_z0 || hi > S.in_z0 + S.in_planes)) return hipErrorInvalidValue;
    if (S.out_float && (S.out_planes < 1 || S.z_begin < S.out_z0 || S.z_end > S.out_z0 + S.out_planes)) return hipErrorInvalidValue;
    return S.bytes_per_voxel == 1 ? launch_smooth_u8(S, st) : launch_smooth_u16(S, st);
}
#endif

}  // namespace vr
