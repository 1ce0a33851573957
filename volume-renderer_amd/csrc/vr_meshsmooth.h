// vr_meshsmooth.h -- host-callable launchers of the mesh smoothing kernels (vr_meshsmooth.hip, vr_smooth_mesh): Taubin's
// lambda|mu filter on the resident mesh's vertex graph and the normals of the result.  The definition, step by step, is in
// include/vr_core.h and DESIGN.md section 1.8; tests/mesh_smooth_ref/mesh_smooth_ref.c restates it on the CPU.
// smooth_mesh (mesh_smooth.cpp) owns the arrays and the order of the launches, the sorts and scans between them are
// vr_primitives.h's; nothing here allocates or waits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vr {

constexpr uint64_t kMeshSmoothMaxPairs = 0xffffffffull;   // 6 T: pair numbers and row offsets are 32-bit
constexpr uint64_t kMeshSmoothIgnoredPair = ~0ull;        // the key of a pair with equal ends: sorts last, belongs to no row

// key[6 t + q] = a << vb | b for the six directed pairs of triangle t (vb = the bits of nv - 1), all ones where a == b
hipError_t launch_meshsmooth_pairs(const uint32_t *triangles, uint64_t nt, uint32_t vb, uint64_t *key, hipStream_t st);
// head[i] = 1 where sorted key i is a pair and differs from key i - 1 (head: n + 1 words, the last one 0); with `fixed` not null
// fixed[a] = 1 for a run of length 1 (fixed: zeroed by the caller; every writer stores the same value)
hipError_t launch_meshsmooth_heads(const uint64_t *key_sorted, uint64_t n, uint32_t vb, uint32_t *head, uint32_t *fixed, hipStream_t st);
// neighbour[offset[i]] = b for every head (offset: head's exclusive sums, n + 1 words) and row[a] = (begin, end) in
// `neighbour` (row: 2 nv words, zeroed by the caller: a vertex without a pair keeps the empty row)
hipError_t launch_meshsmooth_rows(const uint64_t *key_sorted, const uint32_t *offset, uint64_t n, uint32_t vb, uint32_t *neighbour,
                                  uint32_t *row, hipStream_t st);
// the fixed vertices get the empty row, which is what keeps a vertex where it is; *count (zeroed by the caller) = their number
hipError_t launch_meshsmooth_fix(const uint32_t *fixed, uint64_t nv, uint32_t *row, uint32_t *count, hipStream_t st);
// step 4 with factor phi: one thread per vertex, positions [nv][3] in, positions [nv][3] out (in != out)
hipError_t launch_meshsmooth_step(const float *positions_in, float *positions_out, const uint32_t *row, const uint32_t *neighbour, uint64_t nv,
                                  float phi, hipStream_t st);
// step 6, first half: face[t] = (p1 - p0) x (p2 - p0) as four floats; corner_vertex[3 t + q] = the corner's vertex and
// corner_number[3 t + q] = 3 t + q, the pairs whose stable sort by vertex lists every vertex's corners in ascending (t, corner)
hipError_t launch_meshsmooth_faces(const float *positions, const uint32_t *triangles, uint64_t nt, float *face, uint32_t *corner_vertex,
                                   uint32_t *corner_number, hipStream_t st);
// corner_row[v] = (begin, end) of vertex v's run in the sorted corners (2 nv words, zeroed by the caller)
hipError_t launch_meshsmooth_corner_rows(const uint32_t *vertex_sorted, uint64_t n, uint32_t *corner_row, hipStream_t st);
// step 6, second half: normals [nv][3]
hipError_t launch_meshsmooth_normals(const float *face, const uint32_t *corner_row, const uint32_t *number_sorted, uint64_t nv, float *normals,
                                     hipStream_t st);

}  // namespace vr
