// vr_meshsmooth.hip -- smoothing of the resident mesh (vr_smooth_mesh): Taubin's lambda|mu filter -- a Jacobi step towards the
// mean of a vertex's distinct neighbours with factor lambda, then one with factor mu < 0 -- and the normals of the result, the
// normalised sums of the face vectors.  The definition, step by step, is in include/vr_core.h and DESIGN.md section 1.8;
// tests/mesh_smooth_ref/mesh_smooth_ref.c restates it on the CPU and tests/test_mesh_smooth_gpu.py holds these kernels to it bit
// for bit.  No float is ever added atomically: every sum runs in the definition's order inside one thread.
//
// One translation unit: nothing here reads a voxel.  Shape (smooth_mesh, mesh_smooth.cpp, launches them in this order):
//   pairs:    per triangle, its six directed pairs as keys a << vb | b; a pair with equal ends is all ones.
//   sort:     the radix sort (vr_primitives.h) of the keys over the 2 vb bits in use: a vertex's pairs are adjacent, ascending by neighbour,
//             equal pairs in a run whose length is the edge's multiplicity; the ignored pairs come last.
//   heads:    the first of every run; a run of length 1 marks its first end FIXED (its other end is marked by the reverse pair).
//   rows:     an exclusive scan of the heads compacts the neighbours; the first and the last pair of a vertex write its row's
//             begin and end.  A fixed vertex then gets the empty row: one rule, "an empty row copies", keeps it and the isolated.
//   step:     the hot path, 2 * iterations launches: one thread per vertex, positions in the mesh's own 12-byte rows, read from
//             one buffer and written to another; vertices are ordered by voxel, so a wavefront's gathers fall on few lines.
//             (Rows padded to 16 bytes, one aligned load a neighbour, were measured 10 % slower on the largest mesh and 20 % on
//             simplified ones: a quarter more bytes outweigh the rows that straddle two lines.  docs/lab-notebook.md)
//   normals:  the face vectors once (16 bytes a triangle); a stable sort of (vertex, corner number) by vertex lists every vertex's
//             corners in ascending (t, corner); one thread per vertex sums its run and normalises.
// Element numbers are 64-bit and grids two-dimensional: 6 T may be 2^32 - 1.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vr_code_unit.h"
#include "vr_meshsmooth.h"

namespace vr {

namespace {

constexpr uint32_t kGridRow = 1u << 12;
__device__ __forceinline__ uint64_t thread_id() { return ((uint64_t)blockIdx.y * gridDim.x + blockIdx.x) * 256u + threadIdx.x; }
dim3 grid_of(uint64_t threads)
{
    const uint64_t blocks = (threads + 255) / 256;
    return blocks <= kGridRow ? dim3((uint32_t)(blocks ? blocks : 1)) : dim3(kGridRow, (uint32_t)((blocks + kGridRow - 1) / kGridRow));
}

__device__ __forceinline__ uint64_t pair_key(uint32_t a, uint32_t b, uint32_t vb) { return a == b ? kMeshSmoothIgnoredPair : (uint64_t)a << vb | b; }

__global__ __launch_bounds__(256) void meshsmooth_pairs_kernel(const uint32_t *__restrict__ tri, uint64_t nt, uint32_t vb, uint64_t *__restrict__ key)
{
    const uint64_t t = thread_id();
    if (t >= nt) return;
    const uint32_t a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
    uint64_t *const k = key + 6 * t;
    k[0] = pair_key(a, b, vb); k[1] = pair_key(b, a, vb);
    k[2] = pair_key(b, c, vb); k[3] = pair_key(c, b, vb);
    k[4] = pair_key(c, a, vb); k[5] = pair_key(a, c, vb);
}

__global__ __launch_bounds__(256) void meshsmooth_heads_kernel(const uint64_t *__restrict__ key, uint64_t n, uint32_t vb, uint32_t *__restrict__ head,
                                                               uint32_t *fixed)
{
    const uint64_t i = thread_id();
    if (i > n) return;
    uint32_t h = 0;
    if (i < n) {
        const uint64_t k = key[i];
        h = k != kMeshSmoothIgnoredPair && (i == 0 || key[i - 1] != k);
        if (h && fixed && (i + 1 == n || key[i + 1] != k)) fixed[(uint32_t)(k >> vb)] = 1u;   // multiplicity exactly 1
    }
    head[i] = h;
}

__global__ __launch_bounds__(256) void meshsmooth_rows_kernel(const uint64_t *__restrict__ key, const uint32_t *__restrict__ offset, uint64_t n,
                                                              uint32_t vb, uint32_t *__restrict__ neighbour, uint32_t *__restrict__ row)
{
    const uint64_t i = thread_id();
    if (i >= n) return;
    const uint64_t k = key[i];
    if (k == kMeshSmoothIgnoredPair) return;
    const uint32_t a = (uint32_t)(k >> vb), o = offset[i], next = offset[i + 1];
    if (next != o) neighbour[o] = (uint32_t)(k & ((1ull << vb) - 1ull));            // a head
    if (i == 0 || (uint32_t)(key[i - 1] >> vb) != a) row[2ull * a] = o;             // (a key before a pair is a pair)
    if (i + 1 == n || key[i + 1] == kMeshSmoothIgnoredPair || (uint32_t)(key[i + 1] >> vb) != a) row[2ull * a + 1] = next;
}

__global__ __launch_bounds__(256) void meshsmooth_fix_kernel(const uint32_t *__restrict__ fixed, uint64_t nv, uint32_t *__restrict__ row, uint32_t *count)
{
    const uint64_t v = thread_id();
    const bool f = v < nv && fixed[v] != 0;
    if (f) { row[2 * v] = 0u; row[2 * v + 1] = 0u; }
    // every lane takes part in the vote: one atomic per wavefront
    const unsigned long long votes = __ballot(f);
    if ((threadIdx.x & 63u) == 0 && votes) atomicAdd(count, (uint32_t)__popcll(votes));
}

__global__ __launch_bounds__(256) void meshsmooth_step_kernel(const float *__restrict__ in, float *__restrict__ out, const uint2 *__restrict__ row,
                                                              const uint32_t *__restrict__ neighbour, uint64_t nv, float phi)
{
    const uint64_t v = thread_id();
    if (v >= nv) return;
    const uint2 r = row[v];
    float px = in[3 * v], py = in[3 * v + 1], pz = in[3 * v + 2];
    if (r.y != r.x) {
        float ax = 0.0f, ay = 0.0f, az = 0.0f;
        for (uint32_t j = r.x; j < r.y; j++) {
            const float *const q = in + 3ull * neighbour[j];
            ax = ax + q[0]; ay = ay + q[1]; az = az + q[2];
        }
        const float k = (float)(r.y - r.x);
        const float mx = ax / k, my = ay / k, mz = az / k;
        const float dx = mx - px, dy = my - py, dz = mz - pz;
        const float sx = phi * dx, sy = phi * dy, sz = phi * dz;
        px = px + sx; py = py + sy; pz = pz + sz;
    }
    out[3 * v] = px; out[3 * v + 1] = py; out[3 * v + 2] = pz;
}

__global__ __launch_bounds__(256) void meshsmooth_faces_kernel(const float *__restrict__ pos, const uint32_t *__restrict__ tri, uint64_t nt,
                                                               float4 *__restrict__ face, uint32_t *__restrict__ corner_vertex,
                                                               uint32_t *__restrict__ corner_number)
{
    const uint64_t t = thread_id();
    if (t >= nt) return;
    const uint32_t i0 = tri[3 * t], i1 = tri[3 * t + 1], i2 = tri[3 * t + 2];
    const float *const p0 = pos + 3ull * i0, *const p1 = pos + 3ull * i1, *const p2 = pos + 3ull * i2;
    const float ux = p1[0] - p0[0], uy = p1[1] - p0[1], uz = p1[2] - p0[2];
    const float wx = p2[0] - p0[0], wy = p2[1] - p0[1], wz = p2[2] - p0[2];
    const float a0 = uy * wz, b0 = uz * wy, a1 = uz * wx, b1 = ux * wz, a2 = ux * wy, b2 = uy * wx;
    face[t] = make_float4(a0 - b0, a1 - b1, a2 - b2, 0.0f);
    corner_vertex[3 * t] = i0; corner_vertex[3 * t + 1] = i1; corner_vertex[3 * t + 2] = i2;
    const uint32_t q = (uint32_t)(3 * t);
    corner_number[3 * t] = q; corner_number[3 * t + 1] = q + 1u; corner_number[3 * t + 2] = q + 2u;
}

__global__ __launch_bounds__(256) void meshsmooth_corner_rows_kernel(const uint32_t *__restrict__ vertex, uint64_t n, uint32_t *__restrict__ row)
{
    const uint64_t i = thread_id();
    if (i >= n) return;
    const uint32_t v = vertex[i];
    if (i == 0 || vertex[i - 1] != v) row[2ull * v] = (uint32_t)i;
    if (i + 1 == n || vertex[i + 1] != v) row[2ull * v + 1] = (uint32_t)(i + 1);
}

__global__ __launch_bounds__(256) void meshsmooth_normals_kernel(const float4 *__restrict__ face, const uint2 *__restrict__ row,
                                                                 const uint32_t *__restrict__ number, uint64_t nv, float *__restrict__ nrm)
{
    const uint64_t v = thread_id();
    if (v >= nv) return;
    const uint2 r = row[v];
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    for (uint32_t j = r.x; j < r.y; j++) {
        const float4 c = face[number[j] / 3u];
        sx = sx + c.x; sy = sy + c.y; sz = sz + c.z;
    }
    const float zz = sz * sz, yy = sy * sy, xx = sx * sx;
    const float dot = (zz + yy) + xx;
    float nx = 0.0f, ny = 0.0f, nz = 0.0f;
    if (dot != 0.0f) {
        const float rn = 1.0f / sqrtf(dot);
        nx = sx * rn; ny = sy * rn; nz = sz * rn;
    }
    nrm[3 * v] = nx; nrm[3 * v + 1] = ny; nrm[3 * v + 2] = nz;
}

}  // namespace

hipError_t launch_meshsmooth_pairs(const uint32_t *triangles, uint64_t nt, uint32_t vb, uint64_t *key, hipStream_t st)
{
    if (!triangles || !key || nt == 0 || 6 * nt > kMeshSmoothMaxPairs || vb > 32) return hipErrorInvalidValue;
    hipLaunchKernelGGL(meshsmooth_pairs_kernel, grid_of(nt), dim3(256), 0, st, triangles, nt, vb, key);
    return hipGetLastError();
}

hipError_t launch_meshsmooth_heads(const uint64_t *key_sorted, uint64_t n, uint32_t vb, uint32_t *head, uint32_t *fixed, hipStream_t st)
{
    if (!key_sorted || !head || n == 0 || n > kMeshSmoothMaxPairs || vb > 32) return hipErrorInvalidValue;
    hipLaunchKernelGGL(meshsmooth_heads_kernel, grid_of(n + 1), dim3(256), 0, st, key_sorted, n, vb, head, fixed);
    return hipGetLastError();
}

hipError_t launch_meshsmooth_rows(const uint64_t *key_sorted, const uint32_t *offset, uint64_t n, uint32_t vb, uint32_t *neighbour,
                                  uint32_t *row, hipStream_t st)
{
    if (!key_sorted || !offset || !neighbour || !row || n == 0 || n > kMeshSmoothMaxPairs || vb > 32) return hipErrorInvalidValue;
    hipLaunchKernelGGL(meshsmooth_rows_kernel, grid_of(n), dim3(256), 0, st, key_sorted, offset, n, vb, neighbour, row);
    return hipGetLastError();
}

hipError_t launch_meshsmooth_fix(const uint32_t *fixed, uint64_t nv, uint32_t *row, uint32_t *count, hipStream_t st)
{
    if (!fixed || !row || !count || nv == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(meshsmooth_fix_kernel, grid_of(nv), dim3(256), 0, st, fixed, nv, row, count);
    return hipGetLastError();
}

hipError_t launch_meshsmooth_step(const float *positions_in, float *positions_out, const uint32_t *row, const uint32_t *neighbour, uint64_t nv,
                                  float phi, hipStream_t st)
{
    if (!positions_in || !positions_out || positions_in == positions_out || !row || !neighbour || nv == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(meshsmooth_step_kernel, grid_of(nv), dim3(256), 0, st, positions_in, positions_out, (const uint2 *)row, neighbour, nv, phi);
    return hipGetLastError();
}

hipError_t launch_meshsmooth_faces(const float *positions, const uint32_t *triangles, uint64_t nt, float *face, uint32_t *corner_vertex,
                                   uint32_t *corner_number, hipStream_t st)
{
    if (!positions || !triangles || !face || !corner_vertex || !corner_number || nt == 0 || 6 * nt > kMeshSmoothMaxPairs) return hipErrorInvalidValue;
    hipLaunchKernelGGL(meshsmooth_faces_kernel, grid_of(nt), dim3(256), 0, st, positions, triangles, nt, (float4 *)face, corner_vertex,
                       corner_number);
    return hipGetLastError();
}

hipError_t launch_meshsmooth_corner_rows(const uint32_t *vertex_sorted, uint64_t n, uint32_t *corner_row, hipStream_t st)
{
    if (!vertex_sorted || !corner_row || n == 0 || n > kMeshSmoothMaxPairs) return hipErrorInvalidValue;
    hipLaunchKernelGGL(meshsmooth_corner_rows_kernel, grid_of(n), dim3(256), 0, st, vertex_sorted, n, corner_row);
    return hipGetLastError();
}

hipError_t launch_meshsmooth_normals(const float *face, const uint32_t *corner_row, const uint32_t *number_sorted, uint64_t nv, float *normals,
                                     hipStream_t st)
{
    if (!face || !corner_row || !number_sorted || !normals || nv == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(meshsmooth_normals_kernel, grid_of(nv), dim3(256), 0, st, (const float4 *)face, (const uint2 *)corner_row, number_sorted, nv,
                       normals);
    return hipGetLastError();
}

namespace {
VR_CODE_UNIT(meshsmooth, , "mesh smoothing", WARM_LOAD_SHADER)
}  // namespace

}  // namespace vr
