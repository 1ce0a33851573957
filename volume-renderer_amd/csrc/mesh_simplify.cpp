// mesh_simplify.cpp -- simplification of the resident mesh by vertex clustering (vr_simplify_mesh)
#include <algorithm>

#include "volume_ops.h"
#include "vr_primitives.h"
#include "vr_simplify.h"

namespace vr {

// Three stretches of kernels with a read-back after each, because the sizes of what follows depend on it: the extent (the key
// bits; step 2's refusal), the clusters (their number K sizes the winners and the triangles' keys), the kept counts (the new
// mesh).  The arrays of a stretch are freed as soon as nothing reads them.
ResidentMesh simplify_mesh(const DeviceQueue &q, const ResidentMesh &M, float cell, float &ms)
{
    const uint64_t nv = M.nv, nt = M.nt;
    uint64_t new_nv = 0, new_nt = 0;
    DeviceBuffer<float> pos, nrm;                        // the new mesh
    DeviceBuffer<uint32_t> tri;
    if (nv > 0 && nt > 0) {
        const float *const d_pos = M.positions.get(), *const d_nrm = M.normals.get();
        const uint32_t *const d_tri = M.triangles.get();
        GrowingScratch temp("simplifyMesh: hipMalloc(sort scratch)");
        // ---- the extent
        DeviceBuffer<uint32_t> stats;
        stats.allocOrNoMemory(4, "simplifyMesh: hipMalloc(extent)");
        hipError_t e = hipMemsetAsync(stats.get(), 0, 16, q.stream);
        if (e == hipSuccess) e = hipEventRecord(q.ev0, q.stream);
        if (e == hipSuccess) e = launch_simplify_extent(d_pos, nv, cell, stats.get(), q.stream);
        q.check(q.finishTimed(e, ms), "simplification kernels (extent)");
        uint32_t ext[4];
        q.check(hipMemcpy(ext, stats.get(), sizeof(ext), hipMemcpyDeviceToHost), "hipMemcpy(D2H extent)");
        if (ext[3])
            throw RefusalWithMessage("simplifyMesh: a vertex coordinate divided by cell is not in [0, 2^21)",
                                     "The mesh spans 2^21 clustering cells or more along an axis at this cell size. Choose a larger cell.");
        const uint32_t bx = bitWidth(ext[0]), by = bitWidth(ext[1]), bz = bitWidth(ext[2]);
        // ---- the clusters
        DeviceBuffer<uint32_t> cluster, rep;             // per vertex; kept until the mesh is written
        cluster.allocOrNoMemory(nv, "simplifyMesh: hipMalloc(clusters)");
        rep.allocOrNoMemory(nv, "simplifyMesh: hipMalloc(representatives)");
        uint32_t K = 0;
        {
            const uint32_t key_bits = std::max(bx + by + bz, 1u);
            DeviceBuffer<uint64_t> key, key_sorted;
            DeviceBuffer<uint32_t> index, index_sorted, dist, head;
            DeviceBuffer<unsigned long long> winner;
            key.allocOrNoMemory(nv, "simplifyMesh: hipMalloc(keys)");
            key_sorted.allocOrNoMemory(nv, "simplifyMesh: hipMalloc(sorted keys)");
            index.allocOrNoMemory(nv, "simplifyMesh: hipMalloc(indices)");
            index_sorted.allocOrNoMemory(nv, "simplifyMesh: hipMalloc(sorted indices)");
            dist.allocOrNoMemory(nv, "simplifyMesh: hipMalloc(distances)");
            head.allocOrNoMemory(nv, "simplifyMesh: hipMalloc(run heads)");
            const size_t sort_bytes = sort_pairs64_temp_bytes(nv, key_bits), scan_bytes = scan32_temp_bytes(nv);
            temp.atLeast(std::max(sort_bytes, scan_bytes));
            e = hipEventRecord(q.ev0, q.stream);
            if (e == hipSuccess) e = launch_simplify_keys(d_pos, nv, cell, bx, by, key.get(), index.get(), dist.get(), q.stream);
            if (e == hipSuccess) e = launch_sort_pairs64(temp.get(), temp.bytes(), key.get(), key_sorted.get(), index.get(), index_sorted.get(), nv, key_bits, q.stream);
            if (e == hipSuccess) e = launch_simplify_heads(key_sorted.get(), nv, head.get(), q.stream);
            if (e == hipSuccess) e = launch_scan32(head.get(), nv, true, temp.get(), temp.bytes(), q.stream);
            q.check(q.finishTimed(e, ms), "simplification kernels (clusters)");
            q.check(hipMemcpy(&K, head.get() + (nv - 1), sizeof(K), hipMemcpyDeviceToHost), "hipMemcpy(D2H clusters)");
            key.reset(); key_sorted.reset(); index.reset();
            winner.allocOrNoMemory(K, "simplifyMesh: hipMalloc(winners)");
            e = hipMemsetAsync(winner.get(), 0xff, winner.bytes(), q.stream);
            if (e == hipSuccess) e = hipEventRecord(q.ev0, q.stream);
            if (e == hipSuccess) e = launch_simplify_winners(index_sorted.get(), head.get(), dist.get(), nv, cluster.get(), winner.get(), q.stream);
            if (e == hipSuccess) e = launch_simplify_representatives(cluster.get(), winner.get(), nv, rep.get(), q.stream);
            q.check(q.finishTimed(e, ms), "simplification kernels (representatives)");
        }
        // ---- the triangles
        const uint32_t kb = bitWidth(K - 1);
        DeviceBuffer<uint32_t> keep, kept;               // nt + 1 and nv + 1 words: flags, then their exclusive sums
        keep.allocOrNoMemory(nt + 1, "simplifyMesh: hipMalloc(kept triangles)");
        kept.allocOrNoMemory(nv + 1, "simplifyMesh: hipMalloc(kept vertices)");
        {
            DeviceBuffer<uint64_t> ab, ab_ordered, ab_sorted;
            DeviceBuffer<uint32_t> c, c_sorted, index, order1, order2, used;
            ab.allocOrNoMemory(nt, "simplifyMesh: hipMalloc(triples)");
            ab_ordered.allocOrNoMemory(nt, "simplifyMesh: hipMalloc(ordered triples)");
            ab_sorted.allocOrNoMemory(nt, "simplifyMesh: hipMalloc(sorted triples)");
            c.allocOrNoMemory(nt, "simplifyMesh: hipMalloc(third corners)");
            c_sorted.allocOrNoMemory(nt, "simplifyMesh: hipMalloc(sorted third corners)");
            index.allocOrNoMemory(nt, "simplifyMesh: hipMalloc(triangle indices)");
            order1.allocOrNoMemory(nt, "simplifyMesh: hipMalloc(first order)");
            order2.allocOrNoMemory(nt, "simplifyMesh: hipMalloc(second order)");
            used.allocOrNoMemory(K, "simplifyMesh: hipMalloc(used clusters)");
            const uint32_t c_bits = std::max(kb, 1u), ab_bits = std::max(2 * kb, 1u);
            temp.atLeast(std::max(std::max(sort_pairs32_temp_bytes(nt, c_bits), sort_pairs64_temp_bytes(nt, ab_bits)),
                                  std::max(scan32_temp_bytes(nt + 1), scan32_temp_bytes(nv + 1))));
            e = hipMemsetAsync(keep.get(), 0, keep.bytes(), q.stream);
            if (e == hipSuccess) e = hipMemsetAsync(used.get(), 0, used.bytes(), q.stream);
            if (e == hipSuccess) e = hipEventRecord(q.ev0, q.stream);
            if (e == hipSuccess) e = launch_simplify_triples(d_tri, nt, cluster.get(), kb, ab.get(), c.get(), index.get(), q.stream);
            if (e == hipSuccess) e = launch_sort_pairs32(temp.get(), temp.bytes(), c.get(), c_sorted.get(), index.get(), order1.get(), nt, c_bits, q.stream);
            if (e == hipSuccess) e = launch_simplify_gather(ab.get(), order1.get(), nt, ab_ordered.get(), q.stream);
            if (e == hipSuccess) e = launch_sort_pairs64(temp.get(), temp.bytes(), ab_ordered.get(), ab_sorted.get(), order1.get(), order2.get(), nt, ab_bits, q.stream);
            if (e == hipSuccess) e = launch_simplify_keep(ab_sorted.get(), order2.get(), c.get(), nt, kb, keep.get(), used.get(), q.stream);
            if (e == hipSuccess) e = launch_simplify_kept_vertices(rep.get(), cluster.get(), used.get(), nv, kept.get(), q.stream);
            if (e == hipSuccess) e = launch_scan32(keep.get(), nt + 1, false, temp.get(), temp.bytes(), q.stream);
            if (e == hipSuccess) e = launch_scan32(kept.get(), nv + 1, false, temp.get(), temp.bytes(), q.stream);
            q.check(q.finishTimed(e, ms), "simplification kernels (triangles)");
        }
        uint32_t totals[2];
        q.check(hipMemcpy(&totals[0], kept.get() + nv, 4, hipMemcpyDeviceToHost), "hipMemcpy(D2H kept vertices)");
        q.check(hipMemcpy(&totals[1], keep.get() + nt, 4, hipMemcpyDeviceToHost), "hipMemcpy(D2H kept triangles)");
        new_nv = totals[0]; new_nt = totals[1];
        // ---- the new mesh
        if (new_nt > 0) {
            pos.allocOrNoMemory(new_nv * 3, "simplifyMesh: hipMalloc(positions)");
            nrm.allocOrNoMemory(new_nv * 3, "simplifyMesh: hipMalloc(normals)");
            tri.allocOrNoMemory(new_nt * 3, "simplifyMesh: hipMalloc(triangles)");
            e = hipEventRecord(q.ev0, q.stream);
            if (e == hipSuccess) e = launch_simplify_emit_vertices(d_pos, d_nrm, kept.get(), nv, pos.get(), nrm.get(), q.stream);
            if (e == hipSuccess) e = launch_simplify_emit_triangles(d_tri, keep.get(), nt, rep.get(), kept.get(), tri.get(), q.stream);
            q.check(q.finishTimed(e, ms), "simplification kernels (emit)");
        }
    }
    ResidentMesh mesh;
    mesh.adopt(std::move(pos), std::move(nrm), std::move(tri), new_nv, new_nt, M.iso);
    mesh.setSimplified(cell, nv, nt);
    return mesh;
}

}  // namespace vr
