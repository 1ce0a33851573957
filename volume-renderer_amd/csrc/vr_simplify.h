// vr_simplify.h -- host-callable launchers of the mesh simplification kernels (vr_simplify.hip, vr_simplify_mesh): vertex
// clustering on a grid of cubic cells.  The definition, step by step, is in include/vr_core.h and DESIGN.md section 1.7;
// tests/simplify_ref/simplify_ref.c restates it on the CPU.  simplify_mesh (mesh_simplify.cpp) owns the arrays and the order of
// the launches, the sorts and scans between them are vr_primitives.h's; nothing here allocates or waits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vr {

constexpr float kSimplifyMaxQuotient = 2097152.0f;       // 2^21: step 2's bound on p_a / cell, so that three cells pack into 63 bits
constexpr uint64_t kSimplifyMaxCount = 0xffffffffull;     // vertices, triangles: what the mesh's 32-bit indices number

// stats4: zeroed by the caller.  [0 .. 2] = the largest cell index per axis, [3] != 0: a quotient was not in [0, 2^21)
hipError_t launch_simplify_extent(const float *positions, uint64_t nv, float cell, uint32_t *stats4, hipStream_t st);
// key[v] = c_x | c_y << bx | c_z << (bx + by) (bx, by: bits the extent needs), index[v] = v, dist[v] = step 3's dist as bits
hipError_t launch_simplify_keys(const float *positions, uint64_t nv, float cell, uint32_t bx, uint32_t by, uint64_t *key, uint32_t *index,
                                uint32_t *dist, hipStream_t st);
// head[i] = 1 where sorted key i differs from key i - 1 (and at 0): its inclusive sums minus 1 number the clusters in key order
hipError_t launch_simplify_heads(const uint64_t *key_sorted, uint64_t nv, uint32_t *head, hipStream_t st);
// cluster[v] for every vertex, and winner[cluster] = min over its vertices of dist << 32 | v (winner: all bits set by the caller)
hipError_t launch_simplify_winners(const uint32_t *index_sorted, const uint32_t *cluster_sorted, const uint32_t *dist, uint64_t nv,
                                   uint32_t *cluster, unsigned long long *winner, hipStream_t st);
hipError_t launch_simplify_representatives(const uint32_t *cluster, const unsigned long long *winner, uint64_t nv, uint32_t *rep, hipStream_t st);
// per triangle, its corners' clusters a <= b <= c: ab[t] = a << kb | b, c[t], index[t] = t
hipError_t launch_simplify_triples(const uint32_t *triangles, uint64_t nt, const uint32_t *cluster, uint32_t kb, uint64_t *ab, uint32_t *c,
                                   uint32_t *index, hipStream_t st);
hipError_t launch_simplify_gather(const uint64_t *ab, const uint32_t *order, uint64_t nt, uint64_t *ab_ordered, hipStream_t st);
// keep[t] = 1 for the first triangle of every run of equal triples that is not degenerate (keep: nt + 1 words, zeroed by the
// caller), and used[cluster] = 1 for its corners (used: zeroed by the caller)
hipError_t launch_simplify_keep(const uint64_t *ab_sorted, const uint32_t *order, const uint32_t *c, uint64_t nt, uint32_t kb, uint32_t *keep,
                                uint32_t *used, hipStream_t st);
// kept[v] = 1 where v represents its cluster and a kept triangle uses it (kept: nv + 1 words, the last one 0)
hipError_t launch_simplify_kept_vertices(const uint32_t *rep, const uint32_t *cluster, const uint32_t *used, uint64_t nv, uint32_t *kept, hipStream_t st);
// the compactions; vertex_offset and triangle_offset: the exclusive sums of kept and keep (nv + 1, nt + 1 words)
hipError_t launch_simplify_emit_vertices(const float *positions, const float *normals, const uint32_t *vertex_offset, uint64_t nv,
                                         float *out_positions, float *out_normals, hipStream_t st);
hipError_t launch_simplify_emit_triangles(const uint32_t *triangles, const uint32_t *triangle_offset, uint64_t nt, const uint32_t *rep,
                                          const uint32_t *vertex_offset, uint32_t *out_triangles, hipStream_t st);

}  // namespace vr
