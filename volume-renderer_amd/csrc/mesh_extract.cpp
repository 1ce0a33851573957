// mesh_extract.cpp -- isosurface extraction with its mesh (vr_extract_isosurface, vr_extract_components)
#include <algorithm>
#include <vector>

#include "volume_ops.h"
#include "vr_mesh.h"
#include "vr_primitives.h"

namespace vr {

// Two passes over the z slabs the workspace allows.  The first counts and scans every slab and keeps only the slabs' totals: the
// mesh's size is known, and checked, before anything of it is allocated.  The second counts and scans a slab again (not where one
// slab is the whole volume: its arrays are still there) and emits its vertices and triangles at the bases the totals give; a slab
// without a vertex is skipped.  The arrays are freed before this returns.
ResidentMesh extract_mesh(const DeviceQueue &q, const ResidentVolume &V, const float spacing[3], uint64_t workspace_limit, int32_t iso, float iso_s,
                          const uint64_t *selected, float &ms)
{
    const int nx = V.nx, ny = V.ny, nz = V.nz;
    uint64_t nv = 0, nt = 0;
    DeviceBuffer<float> pos, nrm;                        // the new mesh
    DeviceBuffer<uint32_t> tri;
    if (nx >= 2 && ny >= 2 && nz >= 2) {
        const uint64_t plane = (uint64_t)nx * (uint64_t)ny;
        uint64_t bound = workspace_limit;
        if (bound == 0) {
            bound = 2ull << 30;
            uint64_t room = 0;
            if (VolumeCopies::freeBeyondReserve(room)) bound = std::min<uint64_t>(bound, room);
        }
        // planes the arrays hold: a slab's own ones and the plane after them
        uint64_t planes = std::min<uint64_t>(std::min<uint64_t>(bound / (kMeshBytesPerVoxel * plane), kMeshMaxSlabVoxels / plane), (uint64_t)nz);
        if (planes < 2) throw DeviceMemoryError(hipErrorOutOfMemory, "extractIsosurface: the workspace cannot hold two planes of per-voxel counts");
        const int slab = planes >= (uint64_t)nz ? nz : (int)planes - 1;
        const int nslabs = (nz + slab - 1) / slab;
        const uint64_t words = planes * plane + 1;
        const size_t temp_bytes = scan64_temp_bytes(words);
        DeviceBuffer<uint64_t> scan, slab_totals;        // this call's arrays: freed when it returns or throws
        DeviceBuffer<uint8_t> mask, temp;
        scan.allocOrNoMemory(words, "extractIsosurface: hipMalloc(offsets)");
        mask.allocOrNoMemory(planes * plane, "extractIsosurface: hipMalloc(masks)");
        temp.allocOrNoMemory(temp_bytes ? temp_bytes : 16, "extractIsosurface: hipMalloc(scan scratch)");
        slab_totals.allocOrNoMemory((size_t)nslabs * 2, "extractIsosurface: hipMalloc(totals)");
        uint64_t *const d_scan = scan.get(), *const d_totals = slab_totals.get();
        MeshSlab S = {};
        S.volume = V.data; S.bytes_per_voxel = V.bytes_per_voxel; S.layout = V.layout;
        S.nx = nx; S.ny = ny; S.nz = nz;
        S.iso_s = iso_s;
        S.selected = selected;
        for (int a = 0; a < 3; a++) S.spacing[a] = spacing[a];
        S.scan = d_scan; S.mask = mask.get();
        auto countAndScan = [&](int s) {
            S.z0 = s * slab; S.z1 = std::min(S.z0 + slab, nz);
            hipError_t e = launch_mesh_count(S, q.stream);
            if (e == hipSuccess) e = launch_scan64(d_scan, mesh_scan_words(S), temp.get(), temp_bytes, q.stream);
            return e;
        };
        hipError_t e = hipEventRecord(q.ev0, q.stream);
        for (int s = 0; s < nslabs && e == hipSuccess; s++) {
            e = countAndScan(s);
            // vertices of the slab's own planes: the offset of the first voxel after them; triangles: the last word's offset
            if (e == hipSuccess) e = hipMemcpyAsync(d_totals + 2 * s, d_scan + (uint64_t)(S.z1 - S.z0) * plane, sizeof(uint64_t), hipMemcpyDeviceToDevice, q.stream);
            if (e == hipSuccess) e = hipMemcpyAsync(d_totals + 2 * s + 1, d_scan + mesh_scan_words(S) - 1, sizeof(uint64_t), hipMemcpyDeviceToDevice, q.stream);
        }
        q.check(q.finishTimed(e, ms), "extraction kernels (count)");
        std::vector<uint64_t> totals((size_t)nslabs * 2);
        q.check(hipMemcpy(totals.data(), d_totals, totals.size() * sizeof(uint64_t), hipMemcpyDeviceToHost), "hipMemcpy(D2H totals)");
        std::vector<uint64_t> vbase((size_t)nslabs), tbase((size_t)nslabs);
        for (int s = 0; s < nslabs; s++) {
            vbase[s] = nv; tbase[s] = nt;
            nv += totals[2 * s] & 0xffffffffull;
            nt += totals[2 * s + 1] >> 32;
        }
        if (nv > 0xffffffffull || nt > 0xffffffffull)
            throw RefusalWithMessage("extractIsosurface: more than 2^32 - 1 vertices or triangles",
                                     "The isosurface has " + std::to_string(nv) + " vertices and " + std::to_string(nt) +
                                         " triangles: more than 32-bit indices address. Smooth the volume or choose another iso value.");
        if (nv > 0) {
            pos.allocOrNoMemory(nv * 3, "extractIsosurface: hipMalloc(positions)");
            nrm.allocOrNoMemory(nv * 3, "extractIsosurface: hipMalloc(normals)");
        }
        if (nt > 0) tri.allocOrNoMemory(nt * 3, "extractIsosurface: hipMalloc(triangles)");
        if (nv > 0) {
            S.positions = pos.get(); S.normals = nrm.get(); S.triangles = tri.get();
            e = hipEventRecord(q.ev0, q.stream);
            for (int s = 0; s < nslabs && e == hipSuccess; s++) {
                if ((totals[2 * s] & 0xffffffffull) == 0) continue;
                if (nslabs > 1) e = countAndScan(s);
                else { S.z0 = 0; S.z1 = nz; }
                S.vertex_base = vbase[s]; S.triangle_base = tbase[s];
                if (e == hipSuccess) e = launch_mesh_emit(S, q.stream);
            }
            q.check(q.finishTimed(e, ms), "extraction kernels (emit)");
        }
    }
    ResidentMesh mesh;
    mesh.adopt(std::move(pos), std::move(nrm), std::move(tri), nv, nt, iso);
    return mesh;
}

}  // namespace vr
