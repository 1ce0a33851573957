// mesh_smooth.cpp -- smoothing of the resident mesh (vr_smooth_mesh)
#include <algorithm>

#include "volume_ops.h"
#include "vr_meshsmooth.h"
#include "vr_primitives.h"

namespace vr {

// Two timed stretches.  The graph: pairs, their sort, the run heads and their sums, a read-back of the number of distinct pairs
// (it sizes the neighbour array), the rows, the fixed vertices.  Then everything after it: the 2 * iterations steps -- the first
// reads the mesh's positions, the others go between two new buffers -- the face vectors, the sort of the corners, the normals.
// The arrays of a stretch are freed as soon as nothing reads them.
SmoothedMesh smooth_mesh(const DeviceQueue &q, const ResidentMesh &M, int iterations, float lambda, float mu, int fix_boundary, float &build_ms, float &iterate_ms)
{
    const uint64_t nv = M.nv, nt = M.nt;
    if (nt > kMeshSmoothMaxPairs / 6)
        throw RefusalWithMessage("smoothMesh: more than 2^32 - 1 directed pairs",
                                 "The mesh has " + std::to_string(nt) + " triangles: six times that is more than the 32-bit pair numbers of the smoothing "
                                 "address. Simplify the mesh first.");
    SmoothedMesh out;
    if (iterations <= 0 || nv == 0) return out;
    const uint32_t vb = bitWidth(nv - 1);
    const uint64_t np = 6 * nt, nc = 3 * nt;
    DeviceBuffer<float> pos, nrm;                        // the new arrays
    GrowingScratch temp("smoothMesh: hipMalloc(sort scratch)");
    // ---- the graph
    DeviceBuffer<uint32_t> row, neighbour;               // (begin, end) per vertex into the distinct neighbours, ascending within a row
    row.allocOrNoMemory(2 * nv, "smoothMesh: hipMalloc(rows)");
    hipError_t e = hipMemsetAsync(row.get(), 0, row.bytes(), q.stream);
    if (np > 0) {
        DeviceBuffer<uint64_t> key, key_sorted;
        DeviceBuffer<uint32_t> head, fixed, count;
        key.allocOrNoMemory(np, "smoothMesh: hipMalloc(pairs)");
        key_sorted.allocOrNoMemory(np, "smoothMesh: hipMalloc(sorted pairs)");
        head.allocOrNoMemory(np + 1, "smoothMesh: hipMalloc(run heads)");
        if (fix_boundary) {
            fixed.allocOrNoMemory(nv, "smoothMesh: hipMalloc(fixed flags)");
            count.allocOrNoMemory(1, "smoothMesh: hipMalloc(fixed count)");
        }
        const uint32_t key_bits = std::max(2 * vb, 1u);
        temp.atLeast(std::max(sort_keys64_temp_bytes(np, key_bits), scan32_temp_bytes(np + 1)));
        if (e == hipSuccess && fix_boundary) e = hipMemsetAsync(fixed.get(), 0, fixed.bytes(), q.stream);
        if (e == hipSuccess && fix_boundary) e = hipMemsetAsync(count.get(), 0, count.bytes(), q.stream);
        if (e == hipSuccess) e = hipEventRecord(q.ev0, q.stream);
        if (e == hipSuccess) e = launch_meshsmooth_pairs(M.triangles.get(), nt, vb, key.get(), q.stream);
        if (e == hipSuccess) e = launch_sort_keys64(temp.get(), temp.bytes(), key.get(), key_sorted.get(), np, key_bits, q.stream);
        if (e == hipSuccess) e = launch_meshsmooth_heads(key_sorted.get(), np, vb, head.get(), fix_boundary ? fixed.get() : nullptr, q.stream);
        if (e == hipSuccess) e = launch_scan32(head.get(), np + 1, false, temp.get(), temp.bytes(), q.stream);
        q.check(q.finishTimed(e, build_ms), "mesh smoothing kernels (pairs)");
        key.reset();
        uint32_t distinct = 0;
        q.check(hipMemcpy(&distinct, head.get() + np, sizeof(distinct), hipMemcpyDeviceToHost), "hipMemcpy(D2H distinct pairs)");
        neighbour.allocOrNoMemory(std::max<size_t>(distinct, 1), "smoothMesh: hipMalloc(neighbours)");
        e = hipEventRecord(q.ev0, q.stream);
        if (e == hipSuccess) e = launch_meshsmooth_rows(key_sorted.get(), head.get(), np, vb, neighbour.get(), row.get(), q.stream);
        if (e == hipSuccess && fix_boundary) e = launch_meshsmooth_fix(fixed.get(), nv, row.get(), count.get(), q.stream);
        q.check(q.finishTimed(e, build_ms), "mesh smoothing kernels (rows)");
        if (fix_boundary) q.check(hipMemcpy(&out.n_fixed, count.get(), sizeof(out.n_fixed), hipMemcpyDeviceToHost), "hipMemcpy(D2H fixed count)");
    } else {
        neighbour.allocOrNoMemory(1, "smoothMesh: hipMalloc(neighbours)");
        q.check(e, "hipMemset(rows)");
    }
    // ---- the steps
    DeviceBuffer<float> other;                           // pos and other take turns as a step's output
    pos.allocOrNoMemory(3 * nv, "smoothMesh: hipMalloc(positions)");
    if (iterations > 1 || mu != 0.0f) other.allocOrNoMemory(3 * nv, "smoothMesh: hipMalloc(positions)");
    const float *from = M.positions.get();
    e = hipEventRecord(q.ev0, q.stream);
    for (int it = 0; it < iterations && e == hipSuccess; it++)
        for (int half = 0; half < 2 && e == hipSuccess; half++) {
            if (half == 1 && mu == 0.0f) continue;      // plain Laplacian smoothing
            float *const to = from == pos.get() ? other.get() : pos.get();
            e = launch_meshsmooth_step(from, to, row.get(), neighbour.get(), nv, half ? mu : lambda, q.stream);
            from = to;
        }
    q.check(q.finishTimed(e, iterate_ms), "mesh smoothing kernels (steps)");
    row.reset(); neighbour.reset();
    if (from == other.get()) pos.swap(other);           // pos: the result
    other.reset();
    // ---- the normals
    DeviceBuffer<float> face;
    DeviceBuffer<uint32_t> corner_row, vertex, number, vertex_sorted, number_sorted;
    face.allocOrNoMemory(std::max<size_t>(4 * nt, 4), "smoothMesh: hipMalloc(face vectors)");
    corner_row.allocOrNoMemory(2 * nv, "smoothMesh: hipMalloc(corner rows)");
    number_sorted.allocOrNoMemory(std::max<size_t>(nc, 1), "smoothMesh: hipMalloc(sorted corners)");
    nrm.allocOrNoMemory(3 * nv, "smoothMesh: hipMalloc(normals)");
    if (nc > 0) {
        vertex.allocOrNoMemory(nc, "smoothMesh: hipMalloc(corner vertices)");
        number.allocOrNoMemory(nc, "smoothMesh: hipMalloc(corners)");
        vertex_sorted.allocOrNoMemory(nc, "smoothMesh: hipMalloc(sorted corner vertices)");
        temp.atLeast(sort_pairs32_temp_bytes(nc, std::max(vb, 1u)));
    }
    e = hipMemsetAsync(corner_row.get(), 0, corner_row.bytes(), q.stream);
    if (e == hipSuccess) e = hipEventRecord(q.ev0, q.stream);
    if (nc > 0) {
        if (e == hipSuccess) e = launch_meshsmooth_faces(pos.get(), M.triangles.get(), nt, face.get(), vertex.get(), number.get(), q.stream);
        if (e == hipSuccess) e = launch_sort_pairs32(temp.get(), temp.bytes(), vertex.get(), vertex_sorted.get(), number.get(), number_sorted.get(), nc, std::max(vb, 1u), q.stream);
        if (e == hipSuccess) e = launch_meshsmooth_corner_rows(vertex_sorted.get(), nc, corner_row.get(), q.stream);
    }
    if (e == hipSuccess) e = launch_meshsmooth_normals(face.get(), corner_row.get(), number_sorted.get(), nv, nrm.get(), q.stream);
    q.check(q.finishTimed(e, iterate_ms), "mesh smoothing kernels (normals)");
    out.positions = std::move(pos); out.normals = std::move(nrm);
    return out;
}

}  // namespace vr
