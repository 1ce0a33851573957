// vr_simplify.hip -- simplification of the resident mesh by vertex clustering (vr_simplify_mesh): every vertex falls into a
// cubic cell of a grid anchored at the origin, a cell's vertex nearest its centre represents it, triangles are re-indexed to
// the representatives and the collapsed and the repeated ones are dropped.  The definition, step by step, is in
// include/vr_core.h and DESIGN.md section 1.7; tests/simplify_ref/simplify_ref.c restates it on the CPU and
// tests/test_simplify_gpu.py holds these kernels to it bit for bit.
//
// One translation unit: nothing here reads a voxel.  Shape (simplify_mesh, mesh_simplify.cpp, launches them in this order):
//   extent:   per vertex, the three cell indices; their maxima per axis (a fixed grid striding over the vertices, one atomic a
//             wavefront) size the packed key.
//   keys:     per vertex, the packed cell key, the vertex index and the bits of dist.
//   sort:     the stable radix sort (vr_primitives.h) of (key, index) over the key bits in use; run heads + an inclusive scan number the
//             clusters in key order.
//   winners:  a 64-bit atomicMin of dist << 32 | index per cluster: non-negative fp32 bit patterns order like their values
//             and the minimum does not depend on the order of arrival, so the result is the same on every run.
//   triples:  per triangle, its corners' cluster numbers in ascending order.  Cluster numbers are dense, so kb bits each
//             suffice: a stable sort by c, then a stable sort by (a, b) leaves equal triples adjacent in input order.
//   keep:     the first of every run that is not degenerate is kept; its clusters are marked used.
//   emit:     two exclusive scans give the new numbers; one thread per float and per index, so that loads are coalesced and
//             stores go to consecutive addresses.
// Element numbers are 64-bit and grids two-dimensional: a mesh may have 2^32 - 1 triangles, three indices each.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vr_code_unit.h"
#include "vr_simplify.h"

namespace vr {

namespace {

constexpr uint32_t kGridRow = 1u << 12;
__device__ __forceinline__ uint64_t thread_id() { return ((uint64_t)blockIdx.y * gridDim.x + blockIdx.x) * 256u + threadIdx.x; }
dim3 grid_of(uint64_t threads)
{
    const uint64_t blocks = (threads + 255) / 256;
    return blocks <= kGridRow ? dim3((uint32_t)(blocks ? blocks : 1)) : dim3(kGridRow, (uint32_t)((blocks + kGridRow - 1) / kGridRow));
}

// step 2: the cell index on one axis; false where the quotient is not in [0, 2^21)
__device__ __forceinline__ bool cell_of(float p, float cell, uint32_t &c)
{
    const float q = p / cell;
    if (!(q >= 0.0f && q < kSimplifyMaxQuotient)) return false;
    c = (uint32_t)(int32_t)floorf(q);
    return true;
}

// a fixed number of workgroups stride over the vertices, so that the maxima cost kExtentBlocks * 4 * 3 atomics on three addresses
// whatever the mesh's size (one atomic per wavefront of a one-vertex-per-thread grid: 4 ms of a 6.5 ms simplification of 7.5 M vertices)
constexpr uint32_t kExtentBlocks = 1024;

__global__ __launch_bounds__(256) void simplify_extent_kernel(const float *__restrict__ pos, uint64_t nv, float cell, uint32_t *stats)
{
    uint32_t m[3] = {0, 0, 0};
    bool ok = true;
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x; v < nv; v += stride) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            uint32_t c = 0;
            ok = cell_of(pos[3 * v + a], cell, c) && ok;
            m[a] = max(m[a], c);
        }
    }
    // every lane takes part in the reduction: one atomic per wavefront and axis
#pragma unroll
    for (int a = 0; a < 3; a++) {
        uint32_t w = m[a];
        for (int o = 32; o > 0; o >>= 1) w = max(w, (uint32_t)__shfl_xor((int)w, o));
        if ((threadIdx.x & 63u) == 0 && w != 0) atomicMax(&stats[a], w);
    }
    if (!ok) atomicOr(&stats[3], 1u);
}

__global__ __launch_bounds__(256) void simplify_keys_kernel(const float *__restrict__ pos, uint64_t nv, float cell, uint32_t bx, uint32_t by,
                                                            uint64_t *__restrict__ key, uint32_t *__restrict__ index, uint32_t *__restrict__ dist)
{
    const uint64_t v = thread_id();
    if (v >= nv) return;
    uint32_t c[3] = {0, 0, 0};
    float d[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float p = pos[3 * v + a];
        cell_of(p, cell, c[a]);                          // (the extent pass has refused what does not fit)
        const float centre = ((float)c[a] + 0.5f) * cell;
        d[a] = p - centre;
    }
    const float dd = (d[2] * d[2] + d[1] * d[1]) + d[0] * d[0];
    key[v] = (uint64_t)c[0] | (uint64_t)c[1] << bx | (uint64_t)c[2] << (bx + by);
    index[v] = (uint32_t)v;
    dist[v] = __float_as_uint(dd);
}

__global__ __launch_bounds__(256) void simplify_heads_kernel(const uint64_t *__restrict__ key, uint64_t nv, uint32_t *__restrict__ head)
{
    const uint64_t i = thread_id();
    if (i >= nv) return;
    head[i] = i == 0 || key[i] != key[i - 1];
}

__global__ __launch_bounds__(256) void simplify_winners_kernel(const uint32_t *__restrict__ index, const uint32_t *__restrict__ cluster_sorted,
                                                               const uint32_t *__restrict__ dist, uint64_t nv, uint32_t *__restrict__ cluster,
                                                               unsigned long long *winner)
{
    const uint64_t i = thread_id();
    if (i >= nv) return;
    const uint32_t v = index[i], k = cluster_sorted[i] - 1u;
    cluster[v] = k;
    atomicMin(&winner[k], (unsigned long long)dist[v] << 32 | v);
}

__global__ __launch_bounds__(256) void simplify_rep_kernel(const uint32_t *__restrict__ cluster, const unsigned long long *__restrict__ winner,
                                                           uint64_t nv, uint32_t *__restrict__ rep)
{
    const uint64_t v = thread_id();
    if (v >= nv) return;
    rep[v] = (uint32_t)winner[cluster[v]];
}

__global__ __launch_bounds__(256) void simplify_triples_kernel(const uint32_t *__restrict__ tri, uint64_t nt, const uint32_t *__restrict__ cluster,
                                                               uint32_t kb, uint64_t *__restrict__ ab, uint32_t *__restrict__ cc,
                                                               uint32_t *__restrict__ index)
{
    const uint64_t t = thread_id();
    if (t >= nt) return;
    uint32_t a = cluster[tri[3 * t]], b = cluster[tri[3 * t + 1]], c = cluster[tri[3 * t + 2]];
    if (a > b) { const uint32_t x = a; a = b; b = x; }
    if (b > c) { const uint32_t x = b; b = c; c = x; }
    if (a > b) { const uint32_t x = a; a = b; b = x; }
    ab[t] = (uint64_t)a << kb | b;
    cc[t] = c;
    index[t] = (uint32_t)t;
}

__global__ __launch_bounds__(256) void simplify_gather_kernel(const uint64_t *__restrict__ ab, const uint32_t *__restrict__ order, uint64_t nt,
                                                              uint64_t *__restrict__ out)
{
    const uint64_t i = thread_id();
    if (i >= nt) return;
    out[i] = ab[order[i]];
}

__global__ __launch_bounds__(256) void simplify_keep_kernel(const uint64_t *__restrict__ ab, const uint32_t *__restrict__ order,
                                                            const uint32_t *__restrict__ cc, uint64_t nt, uint32_t kb, uint32_t *__restrict__ keep,
                                                            uint32_t *used)
{
    const uint64_t i = thread_id();
    if (i >= nt) return;
    const uint64_t key = ab[i];
    const uint32_t t = order[i], c = cc[t];
    const uint32_t a = (uint32_t)(key >> kb), b = (uint32_t)(key & ((1ull << kb) - 1ull));
    if (!(a < b && b < c)) return;                       // two corners in one cluster: dropped
    if (i > 0 && key == ab[i - 1] && c == cc[order[i - 1]]) return;   // the same vertex set as an earlier triangle
    keep[t] = 1u;
    used[a] = 1u; used[b] = 1u; used[c] = 1u;            // (every writer stores the same value)
}

__global__ __launch_bounds__(256) void simplify_kept_vertices_kernel(const uint32_t *__restrict__ rep, const uint32_t *__restrict__ cluster,
                                                                     const uint32_t *__restrict__ used, uint64_t nv, uint32_t *__restrict__ kept)
{
    const uint64_t v = thread_id();
    if (v > nv) return;
    kept[v] = v < nv && rep[v] == (uint32_t)v && used[cluster[v]] != 0;
}

__global__ __launch_bounds__(256) void simplify_emit_vertices_kernel(const float *__restrict__ pos, const float *__restrict__ nrm,
                                                                     const uint32_t *__restrict__ offset, uint64_t nv, float *__restrict__ out_pos,
                                                                     float *__restrict__ out_nrm)
{
    const uint64_t g = thread_id();
    if (g >= 3 * nv) return;
    const uint64_t v = g / 3;
    const uint32_t o = offset[v];
    if (offset[v + 1] == o) return;
    const uint64_t to = 3ull * o + (g - 3 * v);
    out_pos[to] = pos[g];
    out_nrm[to] = nrm[g];
}

__global__ __launch_bounds__(256) void simplify_emit_triangles_kernel(const uint32_t *__restrict__ tri, const uint32_t *__restrict__ offset,
                                                                      uint64_t nt, const uint32_t *__restrict__ rep,
                                                                      const uint32_t *__restrict__ vertex_offset, uint32_t *__restrict__ out)
{
    const uint64_t g = thread_id();
    if (g >= 3 * nt) return;
    const uint64_t t = g / 3;
    const uint32_t o = offset[t];
    if (offset[t + 1] == o) return;
    out[3ull * o + (g - 3 * t)] = vertex_offset[rep[tri[g]]];
}

}  // namespace

hipError_t launch_simplify_extent(const float *positions, uint64_t nv, float cell, uint32_t *stats4, hipStream_t st)
{
    if (!positions || !stats4 || nv == 0 || nv > kSimplifyMaxCount) return hipErrorInvalidValue;
    const uint64_t blocks = (nv + 255) / 256;
    hipLaunchKernelGGL(simplify_extent_kernel, dim3((uint32_t)(blocks < kExtentBlocks ? blocks : kExtentBlocks)), dim3(256), 0, st, positions, nv, cell, stats4);
    return hipGetLastError();
}

hipError_t launch_simplify_keys(const float *positions, uint64_t nv, float cell, uint32_t bx, uint32_t by, uint64_t *key, uint32_t *index,
                                uint32_t *dist, hipStream_t st)
{
    if (!positions || !key || !index || !dist || nv == 0 || nv > kSimplifyMaxCount || bx > 21 || by > 21) return hipErrorInvalidValue;
    hipLaunchKernelGGL(simplify_keys_kernel, grid_of(nv), dim3(256), 0, st, positions, nv, cell, bx, by, key, index, dist);
    return hipGetLastError();
}

hipError_t launch_simplify_heads(const uint64_t *key_sorted, uint64_t nv, uint32_t *head, hipStream_t st)
{
    if (!key_sorted || !head || nv == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(simplify_heads_kernel, grid_of(nv), dim3(256), 0, st, key_sorted, nv, head);
    return hipGetLastError();
}

hipError_t launch_simplify_winners(const uint32_t *index_sorted, const uint32_t *cluster_sorted, const uint32_t *dist, uint64_t nv,
                                   uint32_t *cluster, unsigned long long *winner, hipStream_t st)
{
    if (!index_sorted || !cluster_sorted || !dist || !cluster || !winner || nv == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(simplify_winners_kernel, grid_of(nv), dim3(256), 0, st, index_sorted, cluster_sorted, dist, nv, cluster, winner);
    return hipGetLastError();
}

hipError_t launch_simplify_representatives(const uint32_t *cluster, const unsigned long long *winner, uint64_t nv, uint32_t *rep, hipStream_t st)
{
    if (!cluster || !winner || !rep || nv == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(simplify_rep_kernel, grid_of(nv), dim3(256), 0, st, cluster, winner, nv, rep);
    return hipGetLastError();
}

hipError_t launch_simplify_triples(const uint32_t *triangles, uint64_t nt, const uint32_t *cluster, uint32_t kb, uint64_t *ab, uint32_t *c,
                                   uint32_t *index, hipStream_t st)
{
    if (!triangles || !cluster || !ab || !c || !index || nt == 0 || nt > kSimplifyMaxCount || kb > 32) return hipErrorInvalidValue;
    hipLaunchKernelGGL(simplify_triples_kernel, grid_of(nt), dim3(256), 0, st, triangles, nt, cluster, kb, ab, c, index);
    return hipGetLastError();
}

hipError_t launch_simplify_gather(const uint64_t *ab, const uint32_t *order, uint64_t nt, uint64_t *ab_ordered, hipStream_t st)
{
    if (!ab || !order || !ab_ordered || nt == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(simplify_gather_kernel, grid_of(nt), dim3(256), 0, st, ab, order, nt, ab_ordered);
    return hipGetLastError();
}

hipError_t launch_simplify_keep(const uint64_t *ab_sorted, const uint32_t *order, const uint32_t *c, uint64_t nt, uint32_t kb, uint32_t *keep,
                                uint32_t *used, hipStream_t st)
{
    if (!ab_sorted || !order || !c || !keep || !used || nt == 0 || kb > 32) return hipErrorInvalidValue;
    hipLaunchKernelGGL(simplify_keep_kernel, grid_of(nt), dim3(256), 0, st, ab_sorted, order, c, nt, kb, keep, used);
    return hipGetLastError();
}

hipError_t launch_simplify_kept_vertices(const uint32_t *rep, const uint32_t *cluster, const uint32_t *used, uint64_t nv, uint32_t *kept, hipStream_t st)
{
    if (!rep || !cluster || !used || !kept || nv == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(simplify_kept_vertices_kernel, grid_of(nv + 1), dim3(256), 0, st, rep, cluster, used, nv, kept);
    return hipGetLastError();
}

hipError_t launch_simplify_emit_vertices(const float *positions, const float *normals, const uint32_t *vertex_offset, uint64_t nv,
                                         float *out_positions, float *out_normals, hipStream_t st)
{
    if (!positions || !normals || !vertex_offset || !out_positions || !out_normals || nv == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(simplify_emit_vertices_kernel, grid_of(3 * nv), dim3(256), 0, st, positions, normals, vertex_offset, nv, out_positions, out_normals);
    return hipGetLastError();
}

hipError_t launch_simplify_emit_triangles(const uint32_t *triangles, const uint32_t *triangle_offset, uint64_t nt, const uint32_t *rep,
                                          const uint32_t *vertex_offset, uint32_t *out_triangles, hipStream_t st)
{
    if (!triangles || !triangle_offset || !rep || !vertex_offset || !out_triangles || nt == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(simplify_emit_triangles_kernel, grid_of(3 * nt), dim3(256), 0, st, triangles, triangle_offset, nt, rep, vertex_offset, out_triangles);
    return hipGetLastError();
}

namespace {
VR_CODE_UNIT(simplify, , "simplification", WARM_LOAD_SHADER)
}  // namespace

}  // namespace vr
