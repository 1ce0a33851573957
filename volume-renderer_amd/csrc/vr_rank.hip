// vr_rank.hip -- grey-level morphology and the median of the resident volume (vr_rank_filter_volume).  The definition is in
// include/vr_core.h and DESIGN.md section 1.9; tests/rank_ref/rank_ref.c restates it on the CPU by brute force and
// tests/test_rank_filter_gpu.py holds these kernels to it bit for bit.
//
// Its own translation units (VR_RANK_TU = 0: 8-bit volumes and the entry point, 1: 16-bit volumes), like vr_smooth.hip, whose
// shape carries over: 256-thread workgroups that stage their input in LDS once and produce a quad along x per lane and output
// row, one vector store each.
//   min / max along x: a workgroup owns 128 x 4 x 4 outputs (whole bricks of a bricked volume) and stages the 16 rows with a
//      halo of two quads on either side.
//   min / max along y, z: a workgroup owns 64 x 4 outputs across the axis and MARCHES along it, 16 rows per step, through a ring
//      of 32 rows in LDS: a row is read from memory once per workgroup (the halo again only where two segments meet).
//   median: one launch; a workgroup owns 64 x 8 x 8 outputs, stages them with a one-voxel halo and selects per output.
// Everything is integer: LDS holds voxels in their own type, registers hold them as 16-bit lanes of a quad (packed unsigned
// min / max; an 8-bit voxel is widened, never a signed compare), staging reads whole quads where a quad lies inside the volume
// and is aligned.  Every load clamps its coordinates into the volume (that IS the edge rule), every store is guarded by the
// volume, index arithmetic is 64-bit throughout.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vr_code_unit.h"
#include "vr_frame.h"
#include "vr_rank.h"

#ifndef VR_RANK_TU
#error "VR_RANK_TU: the unit number comes from the build"
#endif

namespace vr {

namespace {

struct RankArgs {
    const void *in;
    void *out;
    uint32_t nx, ny, nz, bnx, bny;
    int32_t layout;
    int32_t r;                                           // min / max passes
    int32_t seg;                                         // y, z passes: outputs along the axis per workgroup (a multiple of 16)
};

typedef uint16_t quad __attribute__((ext_vector_type(4)));      // four voxels along x in registers, whatever the voxel type
template <typename T> struct Stored;
template <> struct Stored<uint8_t> { typedef uint8_t type __attribute__((ext_vector_type(4))); };
template <> struct Stored<uint16_t> { typedef uint16_t type __attribute__((ext_vector_type(4))); };

__device__ __forceinline__ uint64_t voxel_index(const RankArgs &A, uint32_t i, uint32_t j, uint32_t k)
{
    if (A.layout == 0) return (uint64_t)i + (uint64_t)A.nx * ((uint64_t)j + (uint64_t)A.ny * (uint64_t)k);
    const uint64_t brick = (uint64_t)(i >> BRICK_LX) + (uint64_t)A.bnx * ((uint64_t)(j >> BRICK_LY) + (uint64_t)A.bny * (uint64_t)(k >> BRICK_LZ));
    return brick * 64u + ((i & (BRICK_X - 1u)) | ((j & (BRICK_Y - 1u)) << BRICK_LX) | ((k & (BRICK_Z - 1u)) << (BRICK_LX + BRICK_LY)));
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <bool MAX> __device__ __forceinline__ quad pick(quad a, quad b) { return MAX ? __builtin_elementwise_max(a, b) : __builtin_elementwise_min(a, b); }
template <bool MAX> __device__ __forceinline__ uint32_t pick(uint32_t a, uint32_t b) { return MAX ? (a > b ? a : b) : (a < b ? a : b); }

// in[clamp(x .. x + 3), y, z]: x is a multiple of 4 and may lie outside the volume on either side, y and z are inside
template <typename T>
__device__ __forceinline__ quad load_quad(const RankArgs &A, int x, int y, int z)
{
    typedef typename Stored<T>::type T4;
    const T *in = static_cast<const T *>(A.in);
    if (x >= 0 && x + 4 <= (int)A.nx) {
        // a quad starts a brick row (BRICK_X == 4) or, in the linear layout, lies in one row of the volume: contiguous either way
        const T *p = in + voxel_index(A, (uint32_t)x, (uint32_t)y, (uint32_t)z);
        if (((uintptr_t)p & (4 * sizeof(T) - 1)) == 0) return __builtin_convertvector(*reinterpret_cast<const T4 *>(p), quad);
        return quad{p[0], p[1], p[2], p[3]};
    }
    quad v;
#pragma unroll
    for (int e = 0; e < 4; e++) v[e] = in[voxel_index(A, (uint32_t)clampi(x + e, 0, (int)A.nx - 1), (uint32_t)y, (uint32_t)z)];
    return v;
}

// four outputs at (x .. x + 3, y, z); x is a multiple of 4, and x, y, z are inside the volume
template <typename T>
__device__ __forceinline__ void store_quad(const RankArgs &A, int x, int y, int z, quad v)
{
    typedef typename Stored<T>::type T4;
    const int n = (int)A.nx - x < 4 ? (int)A.nx - x : 4;
    T *o = static_cast<T *>(A.out) + voxel_index(A, (uint32_t)x, (uint32_t)y, (uint32_t)z);
    if (n == 4 && ((uintptr_t)o & (4 * sizeof(T) - 1)) == 0) {
        *reinterpret_cast<T4 *>(o) = __builtin_convertvector(v, T4);
    } else {
        for (int m = 0; m < n; m++) o[m] = (T)v[m];
    }
}
static_assert(BRICK_X == 4, "load_quad and store_quad move one brick row per quad");

// The four windows [m, m + 2r], m = 0 .. 3, over the 2r + 4 values at(0 .. 2r + 3): the values 3 .. 2r lie in all four and are
// reduced once; each output adds the three of its window that are not.
template <bool MAX, typename V, typename At>
__device__ __forceinline__ void four_windows(int r, At at, V out[4])
{
    const V e0 = at(0), e1 = at(1), e2 = at(2);
    const V f1 = at(2 * r + 1), f2 = at(2 * r + 2), f3 = at(2 * r + 3);
    out[0] = pick<MAX>(pick<MAX>(e0, e1), e2);
    out[1] = pick<MAX>(pick<MAX>(e1, e2), f1);
    out[2] = pick<MAX>(pick<MAX>(e2, f1), f2);
    out[3] = pick<MAX>(pick<MAX>(f1, f2), f3);
    if (r >= 2) {                                        // (r == 1: 3 .. 2 is empty and f1 is at(3))
        V c = at(3);
        for (int p = 4; p <= 2 * r; p++) c = pick<MAX>(c, at(p));
#pragma unroll
        for (int m = 0; m < 4; m++) out[m] = pick<MAX>(out[m], c);
    }
}

// ------------------------------------------------------------------ minimum / maximum along x
constexpr int kXTile = 128, kXRows = 16, kXHalo = 8, kXStride = kXTile + 2 * kXHalo;   // 36 quads a row
static_assert(kXHalo >= kRankMaxRadius && kXHalo % 4 == 0, "the staged halo holds the largest radius in whole quads");

template <typename T, bool MAX>
__global__ __launch_bounds__(256) void rank_x_kernel(const RankArgs A)
{
    typedef typename Stored<T>::type T4;
    __shared__ __attribute__((aligned(16))) T s[kXRows * kXStride];
    const int tiles_x = ((int)A.nx + kXTile - 1) / kXTile;
    const int x0 = (int)(blockIdx.x % (uint32_t)tiles_x) * kXTile, y0 = (int)(blockIdx.x / (uint32_t)tiles_x) * 4;
    const int z0 = (int)blockIdx.y * 4;
    const int r = A.r;
    for (int idx = (int)threadIdx.x; idx < kXRows * (kXStride / 4); idx += 256) {
        const int row = idx / (kXStride / 4), p = 4 * (idx % (kXStride / 4));
        if (p + 3 < kXHalo - r || p > kXHalo + kXTile - 1 + r) continue;       // no output reads this quad
        const int y = min(y0 + (row & 3), (int)A.ny - 1), z = min(z0 + (row >> 2), (int)A.nz - 1);
        *reinterpret_cast<T4 *>(&s[row * kXStride + p]) = __builtin_convertvector(load_quad<T>(A, x0 - kXHalo + p, y, z), T4);
    }
    __syncthreads();
    const int xq = (int)threadIdx.x & 31;
    for (int h = 0; h < 2; h++) {
        const int row = ((int)threadIdx.x >> 5) + 8 * h;
        const T *w = &s[row * kXStride + kXHalo + 4 * xq - r];                 // at(p) = the voxel x + p - r
        uint32_t o[4];
        four_windows<MAX, uint32_t>(r, [&](int p) { return (uint32_t)w[p]; }, o);
        const int x = x0 + 4 * xq, y = y0 + (row & 3), z = z0 + (row >> 2);
        if (x < (int)A.nx && y < (int)A.ny && z < (int)A.nz)
            store_quad<T>(A, x, y, z, quad{(uint16_t)o[0], (uint16_t)o[1], (uint16_t)o[2], (uint16_t)o[3]});
    }
}

// ------------------------------------------------------------------ minimum / maximum along y and z
// AXIS 1: a = y, b = z.  AXIS 2: a = z, b = y.  The ring holds a step's 16 rows and both halos: 16 + 2 * 8 rows of 4 x 64 voxels.
constexpr int kRing = 32;
static_assert(16 + 2 * kRankMaxRadius <= kRing && (kRing & (kRing - 1)) == 0, "the ring holds a step's 16 rows and both halos");

template <typename T, bool MAX, int AXIS>
__global__ __launch_bounds__(256) void rank_col_kernel(const RankArgs A)
{
    typedef typename Stored<T>::type T4;
    __shared__ __attribute__((aligned(16))) T ring[kRing * 256];
    const int tiles_x = ((int)A.nx + 63) / 64;
    const int x0 = (int)(blockIdx.x % (uint32_t)tiles_x) * 64;
    const int b_end = AXIS == 1 ? (int)A.nz : (int)A.ny, a_dim = AXIS == 1 ? (int)A.ny : (int)A.nz;
    const int b0 = (int)(blockIdx.x / (uint32_t)tiles_x) * 4;
    const int seg0 = (int)blockIdx.y * A.seg, seg1 = min(seg0 + A.seg, a_dim);
    const int r = A.r;
    // staging: row `ar` of the ring's numbering is a = seg0 - r + ar; 64 threads stage one row of 4 x 16 quads, four rows at a time
    const int sq = (int)threadIdx.x & 63, sr = (int)threadIdx.x >> 6;
    const int lx = x0 + 4 * (sq & 15), lb = min(b0 + (sq >> 4), b_end - 1);
    auto stage = [&](int ar) {
        const int a = clampi(seg0 - r + ar, 0, a_dim - 1);
        const quad v = AXIS == 1 ? load_quad<T>(A, lx, a, lb) : load_quad<T>(A, lx, lb, a);
        *reinterpret_cast<T4 *>(&ring[(ar & (kRing - 1)) * 256 + 4 * sq]) = __builtin_convertvector(v, T4);
    };
    for (int ar = sr; ar < 2 * r; ar += 4) stage(ar);
    const int xq = (int)threadIdx.x & 15, bb = ((int)threadIdx.x >> 4) & 3, aq = (int)threadIdx.x >> 6;
    for (int a0 = seg0; a0 < seg1; a0 += 16) {
        const int base = a0 - seg0;
#pragma unroll
        for (int i = 0; i < 4; i++) stage(base + 2 * r + 4 * i + sr);
        __syncthreads();
        quad o[4];
        four_windows<MAX, quad>(r, [&](int p) {
            return __builtin_convertvector(*reinterpret_cast<const T4 *>(&ring[((base + 4 * aq + p) & (kRing - 1)) * 256 + bb * 64 + 4 * xq]), quad);
        }, o);
        const int x = x0 + 4 * xq, b = b0 + bb;
        if (x < (int)A.nx && b < b_end) {
#pragma unroll
            for (int m = 0; m < 4; m++) {
                const int a = a0 + 4 * aq + m;
                if (a < seg1) {
                    if (AXIS == 1) store_quad<T>(A, x, a, b, o[m]);
                    else store_quad<T>(A, x, b, a, o[m]);
                }
            }
        }
        __syncthreads();                                 // the next step's rows overwrite the oldest ones
    }
}

// ------------------------------------------------------------------ the median over a box of radii 0 or 1
constexpr int kMedX = 64, kMedY = 8, kMedZ = 8, kMedStride = kMedX + 8;        // a quad of halo on either side of a row

__device__ __forceinline__ void order(quad &a, quad &b)
{
    const quad lo = __builtin_elementwise_min(a, b), hi = __builtin_elementwise_max(a, b);
    a = lo; b = hi;
}

// The element at position (N - 1) / 2 of v[0 .. N - 1] in ascending order, by forgetful selection: of any N / 2 + 2 of the values
// neither the smallest nor the largest is the median, and without those two the rest has the same median; so keep a working set,
// move its minimum to the front and its maximum to the back, drop both, take in the next value, until three are left.  Exact
// with equal values: a drop removes one element of the multiset, never a value.
template <int N>
__device__ __forceinline__ quad median_of(const quad (&v)[N])
{
    constexpr int K = N / 2 + 2;
    quad w[K];
#pragma unroll
    for (int i = 0; i < K; i++) w[i] = v[i];
    int next = K;
#pragma unroll
    for (int m = K; m >= 3; m--) {
        const int h = m / 2;
#pragma unroll
        for (int i = 0; i < h; i++) order(w[i], w[m - 1 - i]);                 // the minimum is now in w[0 .. h) or the middle
#pragma unroll
        for (int i = 1; i < h; i++) order(w[0], w[i]);
#pragma unroll
        for (int i = m - h; i < m - 1; i++) order(w[i], w[m - 1]);
        if (m & 1) {
            order(w[0], w[h]);
            order(w[h], w[m - 1]);
        }
        if (m > 3) w[0] = v[next++];                     // w[m - 1] leaves with the shorter set
    }
    return w[1];
}

template <typename T, int RX, int RY, int RZ>
__global__ __launch_bounds__(256) void rank_median_kernel(const RankArgs A)
{
    typedef typename Stored<T>::type T4;
    constexpr int N = (2 * RX + 1) * (2 * RY + 1) * (2 * RZ + 1);
    constexpr int SY = kMedY + 2 * RY, SZ = kMedZ + 2 * RZ, QX = kMedStride / 4;
    __shared__ __attribute__((aligned(16))) T s[SZ * SY * kMedStride];
    const int tiles_x = ((int)A.nx + kMedX - 1) / kMedX;
    const int x0 = (int)(blockIdx.x % (uint32_t)tiles_x) * kMedX, y0 = (int)(blockIdx.x / (uint32_t)tiles_x) * kMedY;
    const int z0 = (int)blockIdx.y * kMedZ;
    for (int idx = (int)threadIdx.x; idx < SZ * SY * QX; idx += 256) {
        const int q = idx % QX, row = idx / QX;
        if (RX == 0 && (q == 0 || q == QX - 1)) continue;                      // no halo along x
        const int y = clampi(y0 - RY + row % SY, 0, (int)A.ny - 1), z = clampi(z0 - RZ + row / SY, 0, (int)A.nz - 1);
        *reinterpret_cast<T4 *>(&s[row * kMedStride + 4 * q]) = __builtin_convertvector(load_quad<T>(A, x0 - 4 + 4 * q, y, z), T4);
    }
    __syncthreads();
    for (int idx = (int)threadIdx.x; idx < kMedX / 4 * kMedY * kMedZ; idx += 256) {
        const int xq = idx & 15, yy = (idx >> 4) & 7, zz = idx >> 7;
        const int x = x0 + 4 * xq, y = y0 + yy, z = z0 + zz;
        if (x >= (int)A.nx || y >= (int)A.ny || z >= (int)A.nz) continue;
        quad v[N];
#pragma unroll
        for (int dz = 0; dz <= 2 * RZ; dz++)
#pragma unroll
            for (int dy = 0; dy <= 2 * RY; dy++) {
                const T *p = &s[((zz + dz) * SY + yy + dy) * kMedStride + 4 + 4 * xq];   // the voxel x of the row y + dy - RY, z + dz - RZ
                const quad mid = __builtin_convertvector(*reinterpret_cast<const T4 *>(p), quad);
                const int at = (dz * (2 * RY + 1) + dy) * (2 * RX + 1);
                if (RX == 0) {
                    v[at] = mid;
                } else {
                    const uint16_t left = p[-1], right = p[4];
                    v[at] = quad{left, mid[0], mid[1], mid[2]};
                    v[at + 1] = mid;
                    v[at + 2] = quad{mid[1], mid[2], mid[3], right};
                }
            }
        store_quad<T>(A, x, y, z, median_of<N>(v));
    }
}
static_assert(kMedX / 4 == 16 && kMedY == 8 && kMedZ == 8, "the median kernel's quad numbering");

template <typename T, bool MAX>
hipError_t launch_minmax(RankArgs A, int axis, hipStream_t st)
{
    if (axis == 0) {
        const uint64_t tiles = (uint64_t)((A.nx + kXTile - 1) / kXTile) * (uint64_t)((A.ny + 3) / 4);
        const uint32_t tz = (A.nz + 3) / 4;
        if (tiles >= (1ull << 31) || tz > 65535u) return hipErrorInvalidValue;
        hipLaunchKernelGGL((rank_x_kernel<T, MAX>), dim3((uint32_t)tiles, tz), dim3(256), 0, st, A);
        return hipGetLastError();
    }
    const int nb = axis == 1 ? (int)A.nz : (int)A.ny, na = axis == 1 ? (int)A.ny : (int)A.nz;
    const uint64_t tiles = (uint64_t)((A.nx + 63) / 64) * (uint64_t)((nb + 3) / 4);
    A.seg = rank_column_segment(na, tiles);
    const uint32_t segs = (uint32_t)((na + A.seg - 1) / A.seg);
    if (tiles >= (1ull << 31) || segs > 65535u) return hipErrorInvalidValue;
    if (axis == 1) hipLaunchKernelGGL((rank_col_kernel<T, MAX, 1>), dim3((uint32_t)tiles, segs), dim3(256), 0, st, A);
    else hipLaunchKernelGGL((rank_col_kernel<T, MAX, 2>), dim3((uint32_t)tiles, segs), dim3(256), 0, st, A);
    return hipGetLastError();
}

template <typename T, int RX, int RY, int RZ>
hipError_t launch_median_box(const RankArgs &A, hipStream_t st)
{
    const uint64_t tiles = (uint64_t)((A.nx + kMedX - 1) / kMedX) * (uint64_t)((A.ny + kMedY - 1) / kMedY);
    const uint32_t tz = (A.nz + kMedZ - 1) / kMedZ;
    if (tiles >= (1ull << 31) || tz > 65535u) return hipErrorInvalidValue;
    hipLaunchKernelGGL((rank_median_kernel<T, RX, RY, RZ>), dim3((uint32_t)tiles, tz), dim3(256), 0, st, A);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_rank_type(const RankPass &P, hipStream_t st)
{
    RankArgs A = {};
    A.in = P.in; A.out = P.out;
    A.nx = (uint32_t)P.nx; A.ny = (uint32_t)P.ny; A.nz = (uint32_t)P.nz;
    A.bnx = (uint32_t)((P.nx + BRICK_X - 1) / BRICK_X); A.bny = (uint32_t)((P.ny + BRICK_Y - 1) / BRICK_Y);
    A.layout = P.layout;
    if (P.kernel == RANK_MEDIAN) {
        switch (P.r3[0] | (P.r3[1] << 1) | (P.r3[2] << 2)) {
        case 1: return launch_median_box<T, 1, 0, 0>(A, st);
        case 2: return launch_median_box<T, 0, 1, 0>(A, st);
        case 3: return launch_median_box<T, 1, 1, 0>(A, st);
        case 4: return launch_median_box<T, 0, 0, 1>(A, st);
        case 5: return launch_median_box<T, 1, 0, 1>(A, st);
        case 6: return launch_median_box<T, 0, 1, 1>(A, st);
        default: return launch_median_box<T, 1, 1, 1>(A, st);
        }
    }
    A.r = P.r3[P.axis];
    return P.kernel == RANK_MAX ? launch_minmax<T, true>(A, P.axis, st) : launch_minmax<T, false>(A, P.axis, st);
}

}  // namespace

VR_CODE_UNIT(rank, VR_RANK_TU, "rank filter", WARM_LOAD_SHADER)

#if VR_RANK_TU == 1
hipError_t launch_rank_u16(const RankPass &P, hipStream_t st) { return launch_rank_type<uint16_t>(P, st); }
#else
// the unit of 8-bit volumes also carries the entry point
hipError_t launch_rank_u8(const RankPass &P, hipStream_t st) { return launch_rank_type<uint8_t>(P, st); }
hipError_t launch_rank_u16(const RankPass &P, hipStream_t st);

hipError_t launch_rank_pass(const RankPass &P, hipStream_t st)
{
    if (!P.in || !P.out || P.in == P.out || P.nx <= 0 || P.ny <= 0 || P.nz <= 0 || (P.layout != 0 && P.layout != 1) ||
        (P.bytes_per_voxel != 1 && P.bytes_per_voxel != 2))
        return hipErrorInvalidValue;
    if (P.kernel == RANK_MEDIAN) {
        for (int a = 0; a < 3; a++)
            if (P.r3[a] < 0 || P.r3[a] > kRankMaxMedianRadius) return hipErrorInvalidValue;
        if (P.r3[0] + P.r3[1] + P.r3[2] == 0) return hipErrorInvalidValue;
    } else if ((P.kernel != RANK_MIN && P.kernel != RANK_MAX) || P.axis < 0 || P.axis > 2 || P.r3[P.axis] < 1 || P.r3[P.axis] > kRankMaxRadius) {
        return hipErrorInvalidValue;
    }
    return P.bytes_per_voxel == 1 ? launch_rank_u8(P, st) : launch_rank_u16(P, st);
}
#endif

}  // namespace vr
