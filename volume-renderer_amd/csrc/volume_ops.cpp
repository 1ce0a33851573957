// volume_ops.cpp -- RendererCore members that compute on the resident volume outside a frame: Gaussian smoothing
// (vr_smooth_volume), isosurface extraction with its mesh (vr_extract_isosurface; section 1.5) and the
// connected components with the filtered extraction (vr_label_components, vr_extract_components; section 1.6), the mesh's
// simplification by vertex clustering (vr_simplify_mesh; section 1.7) and its smoothing (vr_smooth_mesh; section 1.8).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <numeric>

#include "renderer_core.h"
#include "vr_components.h"
#include "vr_mesh.h"
#include "vr_meshsmooth.h"
#include "vr_simplify.h"
#include "vr_smooth.h"

namespace vr {

// The kernels of smoothPasses / extractIsosurface run between ev0_ and ev1_ (the events render() times frames with): records ev1_
// unless `e` says a launch failed, waits for the stream either way, and adds the elapsed time to `ms`
hipError_t RendererCore::finishTimed(hipError_t e, float &ms)
{
    if (e == hipSuccess) e = hipEventRecord(ev1_, stream());
    const hipError_t es = hipStreamSynchronize(stream());
    if (e == hipSuccess) e = es;
    float t = 0.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&t, ev0_, ev1_);
    ms += t;
    return e;
}

// ---------------------------------------------------------------- smoothing (vr_smooth_volume)
// The passes of one smoothing, src -> dst (both allocVolume storage in vol_layout_): x, then y, then z, an axis with sigma 0
// skipped.  With one pass the voxels go straight from src to dst.  With more, fp32 planes carry the intermediates: the whole
// volume's where one buffer fits the workspace bound, else z slabs -- the passes before z then also cover the r_z planes on
// either side of the slab, which the z pass reads (every plane of a slab is computed from the same inputs by the same
// operations as in one piece: the result does not depend on the slab size).  The buffers are freed before this returns.
void RendererCore::smoothPasses(const void *src, void *dst, const float sigma[3])
{
    const int nx = res_dims_[0], ny = res_dims_[1], nz = res_dims_[2];
    float w[3][2 * kSmoothMaxRadius + 1];
    int r[3] = {0, 0, 0}, axes[3], n = 0;
    for (int a = 0; a < 3; a++)
        if (sigma[a] > 0.0f) {
            if (!smooth_weights(sigma[a], w[a], 2 * kSmoothMaxRadius + 1, &r[a])) throw std::invalid_argument("smoothVolume: bad sigma");
            axes[n++] = a;
        }
    SmoothPass S = {};
    S.bytes_per_voxel = res_bytes_; S.layout = vol_layout_;
    S.nx = nx; S.ny = ny; S.nz = nz;
    auto pass = [&](int a, const void *in, bool in_float, void *out, bool out_float, int buf_z0, int buf_planes, int z0, int z1) {
        S.in = in; S.out = out; S.in_float = in_float; S.out_float = out_float;
        S.in_z0 = S.out_z0 = buf_z0; S.in_planes = S.out_planes = buf_planes;
        S.axis = a; S.z_begin = z0; S.z_end = z1; S.radius = r[a]; S.weights = w[a];
        return launch_smooth_pass(S, stream());
    };
    last_smooth_ms_ = 0.0f;                               // (lastSmoothMs: the passes, first launch to last)
    if (n == 1) {
        hipError_t e = hipEventRecord(ev0_, stream());
        if (e == hipSuccess) e = pass(axes[0], src, false, dst, false, 0, 0, 0, nz);
        check(finishTimed(e, last_smooth_ms_), "smooth kernel");
        return;
    }
    const int rz = sigma[2] > 0.0f ? r[2] : 0;           // planes either side of a slab the passes before z must cover
    const uint64_t plane_bytes = (uint64_t)nx * (uint64_t)ny * sizeof(float);
    const int nbuf = n - 1;
    uint64_t bound = smooth_workspace_limit;
    if (bound == 0) {
        bound = 2ull << 30;
        uint64_t room = 0;
        if (VolumeCopies::freeBeyondReserve(room)) bound = std::min<uint64_t>(bound, room / (uint64_t)nbuf);
    }
    uint64_t planes = std::min<uint64_t>(bound / plane_bytes, (uint64_t)nz);
    if (planes < (uint64_t)std::min(nz, 2 * rz + 1))
        throw DeviceMemoryError(hipErrorOutOfMemory, "smoothVolume: the workspace cannot hold one slab of fp32 planes");
    const int slab = planes >= (uint64_t)nz ? nz : (int)planes - 2 * rz;      // output planes per slab
    DeviceBuffer<uint8_t> buf[2];
    for (int b = 0; b < nbuf; b++) buf[b].allocOrNoMemory(planes * plane_bytes, "smoothVolume: hipMalloc(fp32 planes)");
    hipError_t e = hipEventRecord(ev0_, stream());
    for (int s0 = 0; s0 < nz && e == hipSuccess; s0 += slab) {
        const int s1 = std::min(s0 + slab, nz), e0 = std::max(s0 - rz, 0), e1 = std::min(s1 + rz, nz);
        const void *in = src;
        for (int k = 0; k < n && e == hipSuccess; k++) {
            const bool last = k == n - 1;
            void *out = last ? dst : buf[k & 1].get();
            e = pass(axes[k], in, k > 0, out, !last, e0, e1 - e0, last ? s0 : e0, last ? s1 : e1);
            in = out;
        }
    }
    check(finishTimed(e, last_smooth_ms_), "smooth kernel");
}

void RendererCore::smoothVolume(float sigma_x, float sigma_y, float sigma_z)
{
    const float sigma[3] = {sigma_x, sigma_y, sigma_z};
    for (float s : sigma)
        if (!std::isfinite(s) || s < 0.0f || s > kSmoothMaxSigma) throw std::invalid_argument("smoothVolume: every sigma must be finite and in [0, 8] voxels");
    requireDevice("smoothVolume");
    if (!d_vol_) throw std::runtime_error("smoothVolume: no dataset loaded");
    check(hipStreamSynchronize(stream()), "hipStreamSynchronize");      // frames in flight read the buffers replaced below
    const bool off = sigma_x == 0.0f && sigma_y == 0.0f && sigma_z == 0.0f;
    if (off && !d_loaded_) return;                                       // rendering the loaded volume already
    // The volume to render next: the loaded one again, or a new buffer the passes fill (freed with `next` if they throw, which waits
    // for them).  It is swapped in first and swapped back if the range scan fails, so a call that throws leaves the handle as it was.
    DeviceBuffer<uint8_t> next;
    if (!off) {
        try {
            next = allocVolumeBuffer(res_dims_[0], res_dims_[1], res_dims_[2], res_bytes_, vol_layout_);
        } catch (const HipError &err) {
            (void)hipGetLastError();
            throw DeviceMemoryError(err.code, std::string("smoothVolume: ") + err.what());
        }
        smoothPasses(d_loaded_ ? d_loaded_.get() : d_vol_.get(), next.get(), sigma);
    }
    DeviceBuffer<uint8_t> &other = off ? d_loaded_ : next;               // after the swap: the volume rendered until now
    const int keep[8] = {min_val, max_val, min_dataset_val, max_dataset_val, exact_min_, exact_max_, 0, 0};
    d_vol_.swap(other);
    try {
        scanDatasetRange();                                              // the ranges of the rendered volume; it also sets the window from the data ...
    } catch (...) {
        (void)hipStreamSynchronize(stream());
        d_vol_.swap(other);
        min_val = keep[0]; max_val = keep[1]; min_dataset_val = keep[2]; max_dataset_val = keep[3]; exact_min_ = keep[4]; exact_max_ = keep[5];
        throw;
    }
    min_val = keep[0]; max_val = keep[1];                                // ... which is the user's and stays; no message, camera and uniforms untouched
    if (off) d_loaded_.reset();                                          // the smoothed volume
    else if (!d_loaded_) d_loaded_ = std::move(next);                    // (else `next` frees the earlier smoothing result)
    for (int a = 0; a < 3; a++) smooth_sigma_[a] = sigma[a];
    dropDerived();                                                       // what a load leaves behind for new voxels
    freeComponents();                                                    // a labelling of the voxels rendered until now
}

// ---------------------------------------------------------------- extraction (vr_extract_isosurface)
uint64_t RendererCore::meshBytes() const { return d_mesh_pos_.bytes() + d_mesh_nrm_.bytes() + d_mesh_tri_.bytes(); }

void RendererCore::freeMesh()
{
    d_mesh_pos_.reset(); d_mesh_nrm_.reset(); d_mesh_tri_.reset();
    mesh_nv_ = mesh_nt_ = 0;
    mesh_valid_ = false;
    clearMeshSmoothing();                                // (a new mesh is unsmoothed)
}

// Two passes over the z slabs the workspace allows.  The first counts and scans every slab and keeps only the slabs' totals: the
// mesh's size is known, and checked, before anything of it is allocated.  The second counts and scans a slab again (not where one
// slab is the whole volume: its arrays are still there) and emits its vertices and triangles at the bases the totals give; a slab
// without a vertex is skipped.  The arrays are freed before this returns; the previous mesh is replaced only at the very end.
void RendererCore::extractIsosurface(int32_t iso, uint64_t *n_vertices, uint64_t *n_triangles)
{
    requireDevice("extractIsosurface");
    if (!d_vol_) throw std::runtime_error("extractIsosurface: no dataset loaded");
    extractMesh(iso, (float)((int64_t)iso + (datasize_bytes == 2 && (quirks & kQuirkU16Offset) ? 1000 : 0)), nullptr, 0.0f, n_vertices, n_triangles);   // isoStored's rule
}

void RendererCore::extractMesh(int32_t iso, float iso_s, const uint64_t *selected, float ms, uint64_t *n_vertices, uint64_t *n_triangles)
{
    const int nx = res_dims_[0], ny = res_dims_[1], nz = res_dims_[2];
    uint64_t nv = 0, nt = 0;
    DeviceBuffer<float> pos, nrm;                        // the new mesh: moved into the handle at the very end
    DeviceBuffer<uint32_t> tri;
    if (nx >= 2 && ny >= 2 && nz >= 2) {
        const uint64_t plane = (uint64_t)nx * (uint64_t)ny;
        uint64_t bound = mesh_workspace_limit;
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
        const size_t temp_bytes = mesh_scan_temp_bytes(words);
        DeviceBuffer<uint64_t> scan, slab_totals;        // this call's arrays: freed when it returns or throws
        DeviceBuffer<uint8_t> mask, temp;
        scan.allocOrNoMemory(words, "extractIsosurface: hipMalloc(offsets)");
        mask.allocOrNoMemory(planes * plane, "extractIsosurface: hipMalloc(masks)");
        temp.allocOrNoMemory(temp_bytes ? temp_bytes : 16, "extractIsosurface: hipMalloc(scan scratch)");
        slab_totals.allocOrNoMemory((size_t)nslabs * 2, "extractIsosurface: hipMalloc(totals)");
        uint64_t *const d_scan = scan.get(), *const d_totals = slab_totals.get();
        MeshSlab S = {};
        S.volume = d_vol_.get(); S.bytes_per_voxel = res_bytes_; S.layout = vol_layout_;
        S.nx = nx; S.ny = ny; S.nz = nz;
        S.iso_s = iso_s;
        S.selected = selected;
        for (int a = 0; a < 3; a++) S.spacing[a] = voxel_size[a];
        S.scan = d_scan; S.mask = mask.get();
        auto countAndScan = [&](int s) {
            S.z0 = s * slab; S.z1 = std::min(S.z0 + slab, nz);
            hipError_t e = launch_mesh_count(S, stream());
            if (e == hipSuccess) e = launch_mesh_scan(d_scan, mesh_scan_words(S), temp.get(), temp_bytes, stream());
            return e;
        };
        hipError_t e = hipEventRecord(ev0_, stream());
        for (int s = 0; s < nslabs && e == hipSuccess; s++) {
            e = countAndScan(s);
            // vertices of the slab's own planes: the offset of the first voxel after them; triangles: the last word's offset
            if (e == hipSuccess) e = hipMemcpyAsync(d_totals + 2 * s, d_scan + (uint64_t)(S.z1 - S.z0) * plane, sizeof(uint64_t), hipMemcpyDeviceToDevice, stream());
            if (e == hipSuccess) e = hipMemcpyAsync(d_totals + 2 * s + 1, d_scan + mesh_scan_words(S) - 1, sizeof(uint64_t), hipMemcpyDeviceToDevice, stream());
        }
        check(finishTimed(e, ms), "extraction kernels (count)");
        std::vector<uint64_t> totals((size_t)nslabs * 2);
        check(hipMemcpy(totals.data(), d_totals, totals.size() * sizeof(uint64_t), hipMemcpyDeviceToHost), "hipMemcpy(D2H totals)");
        std::vector<uint64_t> vbase((size_t)nslabs), tbase((size_t)nslabs);
        for (int s = 0; s < nslabs; s++) {
            vbase[s] = nv; tbase[s] = nt;
            nv += totals[2 * s] & 0xffffffffull;
            nt += totals[2 * s + 1] >> 32;
        }
        if (nv > 0xffffffffull || nt > 0xffffffffull) {
            setMessage("Error!", "The isosurface has " + std::to_string(nv) + " vertices and " + std::to_string(nt) +
                                     " triangles: more than 32-bit indices address. Smooth the volume or choose another iso value.");
            throw std::invalid_argument("extractIsosurface: more than 2^32 - 1 vertices or triangles");
        }
        if (nv > 0) {
            pos.allocOrNoMemory(nv * 3, "extractIsosurface: hipMalloc(positions)");
            nrm.allocOrNoMemory(nv * 3, "extractIsosurface: hipMalloc(normals)");
        }
        if (nt > 0) tri.allocOrNoMemory(nt * 3, "extractIsosurface: hipMalloc(triangles)");
        if (nv > 0) {
            S.positions = pos.get(); S.normals = nrm.get(); S.triangles = tri.get();
            e = hipEventRecord(ev0_, stream());
            for (int s = 0; s < nslabs && e == hipSuccess; s++) {
                if ((totals[2 * s] & 0xffffffffull) == 0) continue;
                if (nslabs > 1) e = countAndScan(s);
                else { S.z0 = 0; S.z1 = nz; }
                S.vertex_base = vbase[s]; S.triangle_base = tbase[s];
                if (e == hipSuccess) e = launch_mesh_emit(S, stream());
            }
            check(finishTimed(e, ms), "extraction kernels (emit)");
        }
    }
    freeMesh();
    d_mesh_pos_ = std::move(pos); d_mesh_nrm_ = std::move(nrm); d_mesh_tri_ = std::move(tri);
    mesh_nv_ = nv; mesh_nt_ = nt; mesh_iso_ = iso; mesh_valid_ = true;
    mesh_cell_ = 0.0f; mesh_src_nv_ = nv; mesh_src_nt_ = nt;               // (meshSimplification: not simplified)
    last_mesh_ms_ = ms;
    if (n_vertices) *n_vertices = nv;
    if (n_triangles) *n_triangles = nt;
}

// ---------------------------------------------------------------- simplification (vr_simplify_mesh)
// Three stretches of kernels with a read-back after each, because the sizes of what follows depend on it: the extent (the key
// bits; step 2's refusal), the clusters (their number K sizes the winners and the triangles' keys), the kept counts (the new
// mesh).  The arrays of a stretch are freed as soon as nothing reads them; the new mesh is swapped in at the very end.
void RendererCore::simplifyMesh(float cell, uint64_t *n_vertices, uint64_t *n_triangles)
{
    requireDevice("simplifyMesh");
    if (!std::isnormal(cell) || !(cell > 0.0f)) throw std::invalid_argument("simplifyMesh: cell must be a finite, normal number above 0");
    if (!mesh_valid_) throw std::invalid_argument("simplifyMesh: no isosurface has been extracted");
    const uint64_t nv = mesh_nv_, nt = mesh_nt_;
    uint64_t new_nv = 0, new_nt = 0;
    float ms = 0.0f;
    DeviceBuffer<float> pos, nrm;                        // the new mesh
    DeviceBuffer<uint32_t> tri;
    auto bitsOf = [](uint64_t m) { uint32_t b = 0; while (m) { b++; m >>= 1; } return b; };
    if (nv > 0 && nt > 0) {
        const float *const d_pos = d_mesh_pos_.get(), *const d_nrm = d_mesh_nrm_.get();
        const uint32_t *const d_tri = d_mesh_tri_.get();
        DeviceBuffer<uint8_t> temp;
        auto scratch = [&](size_t bytes) { if (temp.bytes() < bytes || !temp) temp.allocOrNoMemory(bytes ? bytes : 16, "simplifyMesh: hipMalloc(sort scratch)"); };
        // ---- the extent
        DeviceBuffer<uint32_t> stats;
        stats.allocOrNoMemory(4, "simplifyMesh: hipMalloc(extent)");
        hipError_t e = hipMemsetAsync(stats.get(), 0, 16, stream());
        if (e == hipSuccess) e = hipEventRecord(ev0_, stream());
        if (e == hipSuccess) e = launch_simplify_extent(d_pos, nv, cell, stats.get(), stream());
        check(finishTimed(e, ms), "simplification kernels (extent)");
        uint32_t ext[4];
        check(hipMemcpy(ext, stats.get(), sizeof(ext), hipMemcpyDeviceToHost), "hipMemcpy(D2H extent)");
        if (ext[3]) {
            setMessage("Error!", "The mesh spans 2^21 clustering cells or more along an axis at this cell size. Choose a larger cell.");
            throw std::invalid_argument("simplifyMesh: a vertex coordinate divided by cell is not in [0, 2^21)");
        }
        const uint32_t bx = bitsOf(ext[0]), by = bitsOf(ext[1]), bz = bitsOf(ext[2]);
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
            const size_t sort_bytes = simplify_sort64_temp_bytes(nv, key_bits), scan_bytes = simplify_scan_temp_bytes(nv);
            scratch(std::max(sort_bytes, scan_bytes));
            e = hipEventRecord(ev0_, stream());
            if (e == hipSuccess) e = launch_simplify_keys(d_pos, nv, cell, bx, by, key.get(), index.get(), dist.get(), stream());
            if (e == hipSuccess) e = launch_simplify_sort64(temp.get(), temp.bytes(), key.get(), key_sorted.get(), index.get(), index_sorted.get(), nv, key_bits, stream());
            if (e == hipSuccess) e = launch_simplify_heads(key_sorted.get(), nv, head.get(), stream());
            if (e == hipSuccess) e = launch_simplify_scan(head.get(), nv, true, temp.get(), temp.bytes(), stream());
            check(finishTimed(e, ms), "simplification kernels (clusters)");
            check(hipMemcpy(&K, head.get() + (nv - 1), sizeof(K), hipMemcpyDeviceToHost), "hipMemcpy(D2H clusters)");
            key.reset(); key_sorted.reset(); index.reset();
            winner.allocOrNoMemory(K, "simplifyMesh: hipMalloc(winners)");
            e = hipMemsetAsync(winner.get(), 0xff, winner.bytes(), stream());
            if (e == hipSuccess) e = hipEventRecord(ev0_, stream());
            if (e == hipSuccess) e = launch_simplify_winners(index_sorted.get(), head.get(), dist.get(), nv, cluster.get(), winner.get(), stream());
            if (e == hipSuccess) e = launch_simplify_representatives(cluster.get(), winner.get(), nv, rep.get(), stream());
            check(finishTimed(e, ms), "simplification kernels (representatives)");
        }
        // ---- the triangles
        const uint32_t kb = bitsOf(K - 1);
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
            scratch(std::max(std::max(simplify_sort32_temp_bytes(nt, c_bits), simplify_sort64_temp_bytes(nt, ab_bits)),
                             std::max(simplify_scan_temp_bytes(nt + 1), simplify_scan_temp_bytes(nv + 1))));
            e = hipMemsetAsync(keep.get(), 0, keep.bytes(), stream());
            if (e == hipSuccess) e = hipMemsetAsync(used.get(), 0, used.bytes(), stream());
            if (e == hipSuccess) e = hipEventRecord(ev0_, stream());
            if (e == hipSuccess) e = launch_simplify_triples(d_tri, nt, cluster.get(), kb, ab.get(), c.get(), index.get(), stream());
            if (e == hipSuccess) e = launch_simplify_sort32(temp.get(), temp.bytes(), c.get(), c_sorted.get(), index.get(), order1.get(), nt, c_bits, stream());
            if (e == hipSuccess) e = launch_simplify_gather(ab.get(), order1.get(), nt, ab_ordered.get(), stream());
            if (e == hipSuccess) e = launch_simplify_sort64(temp.get(), temp.bytes(), ab_ordered.get(), ab_sorted.get(), order1.get(), order2.get(), nt, ab_bits, stream());
            if (e == hipSuccess) e = launch_simplify_keep(ab_sorted.get(), order2.get(), c.get(), nt, kb, keep.get(), used.get(), stream());
            if (e == hipSuccess) e = launch_simplify_kept_vertices(rep.get(), cluster.get(), used.get(), nv, kept.get(), stream());
            if (e == hipSuccess) e = launch_simplify_scan(keep.get(), nt + 1, false, temp.get(), temp.bytes(), stream());
            if (e == hipSuccess) e = launch_simplify_scan(kept.get(), nv + 1, false, temp.get(), temp.bytes(), stream());
            check(finishTimed(e, ms), "simplification kernels (triangles)");
        }
        uint32_t totals[2];
        check(hipMemcpy(&totals[0], kept.get() + nv, 4, hipMemcpyDeviceToHost), "hipMemcpy(D2H kept vertices)");
        check(hipMemcpy(&totals[1], keep.get() + nt, 4, hipMemcpyDeviceToHost), "hipMemcpy(D2H kept triangles)");
        new_nv = totals[0]; new_nt = totals[1];
        // ---- the new mesh
        if (new_nt > 0) {
            pos.allocOrNoMemory(new_nv * 3, "simplifyMesh: hipMalloc(positions)");
            nrm.allocOrNoMemory(new_nv * 3, "simplifyMesh: hipMalloc(normals)");
            tri.allocOrNoMemory(new_nt * 3, "simplifyMesh: hipMalloc(triangles)");
            e = hipEventRecord(ev0_, stream());
            if (e == hipSuccess) e = launch_simplify_emit_vertices(d_pos, d_nrm, kept.get(), nv, pos.get(), nrm.get(), stream());
            if (e == hipSuccess) e = launch_simplify_emit_triangles(d_tri, keep.get(), nt, rep.get(), kept.get(), tri.get(), stream());
            check(finishTimed(e, ms), "simplification kernels (emit)");
        }
    }
    const int32_t iso = mesh_iso_;
    freeMesh();
    d_mesh_pos_ = std::move(pos); d_mesh_nrm_ = std::move(nrm); d_mesh_tri_ = std::move(tri);
    mesh_nv_ = new_nv; mesh_nt_ = new_nt; mesh_iso_ = iso; mesh_valid_ = true;
    mesh_cell_ = cell; mesh_src_nv_ = nv; mesh_src_nt_ = nt;
    last_simplify_ms_ = ms;
    if (n_vertices) *n_vertices = new_nv;
    if (n_triangles) *n_triangles = new_nt;
}

void RendererCore::meshSimplification(float *cell, uint64_t *source_vertices, uint64_t *source_triangles) const
{
    if (!mesh_valid_) throw std::invalid_argument("meshSimplification: no isosurface has been extracted");
    if (cell) *cell = mesh_cell_;
    if (source_vertices) *source_vertices = mesh_src_nv_;
    if (source_triangles) *source_triangles = mesh_src_nt_;
}

// ---------------------------------------------------------------- mesh smoothing (vr_smooth_mesh)
// Two timed stretches.  The graph: pairs, their sort, the run heads and their sums, a read-back of the number of distinct pairs
// (it sizes the neighbour array), the rows, the fixed vertices.  Then everything after it: the 2 * iterations steps -- the first
// reads the mesh's positions, the others go between two new buffers -- the face vectors, the sort of the corners, the normals.  The arrays of a stretch are
// freed as soon as nothing reads them; the new positions and normals are swapped in at the very end, the triangles stay.
void RendererCore::smoothMesh(int iterations, float lambda, float mu, int fix_boundary)
{
    requireDevice("smoothMesh");
    if (iterations < 0 || iterations > 1000) throw std::invalid_argument("smoothMesh: iterations must be in [0, 1000]");
    if (!std::isfinite(lambda) || !(lambda > 0.0f && lambda <= 1.0f)) throw std::invalid_argument("smoothMesh: lambda must be in (0, 1]");
    if (!std::isfinite(mu) || !(mu >= -2.0f && mu <= 0.0f)) throw std::invalid_argument("smoothMesh: mu must be in [-2, 0]");
    if (!mesh_valid_) throw std::invalid_argument("smoothMesh: no isosurface has been extracted");
    const uint64_t nv = mesh_nv_, nt = mesh_nt_;
    if (nt > kMeshSmoothMaxPairs / 6) {
        setMessage("Error!", "The mesh has " + std::to_string(nt) + " triangles: six times that is more than the 32-bit pair numbers of the smoothing "
                                 "address. Simplify the mesh first.");
        throw std::invalid_argument("smoothMesh: more than 2^32 - 1 directed pairs");
    }
    float build_ms = 0.0f, iterate_ms = 0.0f;
    uint32_t n_fixed = 0;
    if (iterations > 0 && nv > 0) {
        auto bitsOf = [](uint64_t m) { uint32_t b = 0; while (m) { b++; m >>= 1; } return b; };
        const uint32_t vb = bitsOf(nv - 1);
        const uint64_t np = 6 * nt, nc = 3 * nt;
        DeviceBuffer<float> pos, nrm;                    // the new arrays
        DeviceBuffer<uint8_t> temp;
        auto scratch = [&](size_t bytes) { if (temp.bytes() < bytes || !temp) temp.allocOrNoMemory(bytes ? bytes : 16, "smoothMesh: hipMalloc(sort scratch)"); };
        // ---- the graph
        DeviceBuffer<uint32_t> row, neighbour;           // (begin, end) per vertex into the distinct neighbours, ascending within a row
        row.allocOrNoMemory(2 * nv, "smoothMesh: hipMalloc(rows)");
        hipError_t e = hipMemsetAsync(row.get(), 0, row.bytes(), stream());
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
            scratch(std::max(meshsmooth_sort_keys_temp_bytes(np, key_bits), meshsmooth_scan_temp_bytes(np + 1)));
            if (e == hipSuccess && fix_boundary) e = hipMemsetAsync(fixed.get(), 0, fixed.bytes(), stream());
            if (e == hipSuccess && fix_boundary) e = hipMemsetAsync(count.get(), 0, count.bytes(), stream());
            if (e == hipSuccess) e = hipEventRecord(ev0_, stream());
            if (e == hipSuccess) e = launch_meshsmooth_pairs(d_mesh_tri_.get(), nt, vb, key.get(), stream());
            if (e == hipSuccess) e = launch_meshsmooth_sort_keys(temp.get(), temp.bytes(), key.get(), key_sorted.get(), np, key_bits, stream());
            if (e == hipSuccess) e = launch_meshsmooth_heads(key_sorted.get(), np, vb, head.get(), fix_boundary ? fixed.get() : nullptr, stream());
            if (e == hipSuccess) e = launch_meshsmooth_scan(head.get(), np + 1, temp.get(), temp.bytes(), stream());
            check(finishTimed(e, build_ms), "mesh smoothing kernels (pairs)");
            key.reset();
            uint32_t distinct = 0;
            check(hipMemcpy(&distinct, head.get() + np, sizeof(distinct), hipMemcpyDeviceToHost), "hipMemcpy(D2H distinct pairs)");
            neighbour.allocOrNoMemory(std::max<size_t>(distinct, 1), "smoothMesh: hipMalloc(neighbours)");
            e = hipEventRecord(ev0_, stream());
            if (e == hipSuccess) e = launch_meshsmooth_rows(key_sorted.get(), head.get(), np, vb, neighbour.get(), row.get(), stream());
            if (e == hipSuccess && fix_boundary) e = launch_meshsmooth_fix(fixed.get(), nv, row.get(), count.get(), stream());
            check(finishTimed(e, build_ms), "mesh smoothing kernels (rows)");
            if (fix_boundary) check(hipMemcpy(&n_fixed, count.get(), sizeof(n_fixed), hipMemcpyDeviceToHost), "hipMemcpy(D2H fixed count)");
        } else {
            neighbour.allocOrNoMemory(1, "smoothMesh: hipMalloc(neighbours)");
            check(e, "hipMemset(rows)");
        }
        // ---- the steps
        DeviceBuffer<float> other;                       // pos and other take turns as a step's output
        pos.allocOrNoMemory(3 * nv, "smoothMesh: hipMalloc(positions)");
        if (iterations > 1 || mu != 0.0f) other.allocOrNoMemory(3 * nv, "smoothMesh: hipMalloc(positions)");
        const float *from = d_mesh_pos_.get();
        e = hipEventRecord(ev0_, stream());
        for (int it = 0; it < iterations && e == hipSuccess; it++)
            for (int half = 0; half < 2 && e == hipSuccess; half++) {
                if (half == 1 && mu == 0.0f) continue;  // plain Laplacian smoothing
                float *const to = from == pos.get() ? other.get() : pos.get();
                e = launch_meshsmooth_step(from, to, row.get(), neighbour.get(), nv, half ? mu : lambda, stream());
                from = to;
            }
        check(finishTimed(e, iterate_ms), "mesh smoothing kernels (steps)");
        row.reset(); neighbour.reset();
        if (from == other.get()) pos.swap(other);       // pos: the result
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
            scratch(meshsmooth_sort_pairs_temp_bytes(nc, std::max(vb, 1u)));
        }
        e = hipMemsetAsync(corner_row.get(), 0, corner_row.bytes(), stream());
        if (e == hipSuccess) e = hipEventRecord(ev0_, stream());
        if (nc > 0) {
            if (e == hipSuccess) e = launch_meshsmooth_faces(pos.get(), d_mesh_tri_.get(), nt, face.get(), vertex.get(), number.get(), stream());
            if (e == hipSuccess) e = launch_meshsmooth_sort_pairs(temp.get(), temp.bytes(), vertex.get(), vertex_sorted.get(), number.get(), number_sorted.get(), nc, std::max(vb, 1u), stream());
            if (e == hipSuccess) e = launch_meshsmooth_corner_rows(vertex_sorted.get(), nc, corner_row.get(), stream());
        }
        if (e == hipSuccess) e = launch_meshsmooth_normals(face.get(), corner_row.get(), number_sorted.get(), nv, nrm.get(), stream());
        check(finishTimed(e, iterate_ms), "mesh smoothing kernels (normals)");
        d_mesh_pos_ = std::move(pos); d_mesh_nrm_ = std::move(nrm);
    }
    mesh_smooth_iterations_ = iterations; mesh_smooth_lambda_ = lambda; mesh_smooth_mu_ = mu; mesh_smooth_fix_ = fix_boundary != 0;
    mesh_smooth_fixed_ = n_fixed;
    last_mesh_smooth_build_ms_ = build_ms; last_mesh_smooth_iterate_ms_ = iterate_ms;
}

void RendererCore::meshSmoothing(int *iterations, float *lambda, float *mu, int *fix_boundary, uint64_t *fixed_vertices) const
{
    if (!mesh_valid_) throw std::invalid_argument("meshSmoothing: no isosurface has been extracted");
    if (iterations) *iterations = mesh_smooth_iterations_;
    if (lambda) *lambda = mesh_smooth_lambda_;
    if (mu) *mu = mesh_smooth_mu_;
    if (fix_boundary) *fix_boundary = mesh_smooth_fix_ ? 1 : 0;
    if (fixed_vertices) *fixed_vertices = mesh_smooth_fixed_;
}

void RendererCore::clearMeshSmoothing()
{
    mesh_smooth_iterations_ = 0; mesh_smooth_lambda_ = mesh_smooth_mu_ = 0.0f; mesh_smooth_fix_ = false; mesh_smooth_fixed_ = 0;
}

void RendererCore::meshInfo(int32_t *iso, uint64_t *n_vertices, uint64_t *n_triangles) const
{
    if (!mesh_valid_) throw std::invalid_argument("meshInfo: no isosurface has been extracted");
    if (iso) *iso = mesh_iso_;
    if (n_vertices) *n_vertices = mesh_nv_;
    if (n_triangles) *n_triangles = mesh_nt_;
}

void RendererCore::readMesh(float *positions, float *normals, uint32_t *triangles, uint64_t vertex_capacity, uint64_t triangle_capacity)
{
    if (!mesh_valid_) throw std::invalid_argument("readMesh: no isosurface has been extracted");
    if (((positions || normals) && vertex_capacity < mesh_nv_) || (triangles && triangle_capacity < mesh_nt_))
        throw std::invalid_argument("readMesh: buffer too small");
    requireDevice("readMesh");
    if (positions && mesh_nv_) check(hipMemcpyAsync(positions, d_mesh_pos_.get(), mesh_nv_ * 12, hipMemcpyDeviceToHost, stream()), "hipMemcpy(D2H positions)");
    if (normals && mesh_nv_) check(hipMemcpyAsync(normals, d_mesh_nrm_.get(), mesh_nv_ * 12, hipMemcpyDeviceToHost, stream()), "hipMemcpy(D2H normals)");
    if (triangles && mesh_nt_) check(hipMemcpyAsync(triangles, d_mesh_tri_.get(), mesh_nt_ * 12, hipMemcpyDeviceToHost, stream()), "hipMemcpy(D2H triangles)");
    check(hipStreamSynchronize(stream()), "hipStreamSynchronize");
}

// "stl": binary STL, the facet normal the unit cross product of the stored positions in double, (0, 0, 0) for a zero-area
// triangle, attribute word 0.  "ply": binary_little_endian 1.0, x y z nx ny nz as float, faces uchar uint.
void RendererCore::saveMesh(const std::string &fn, const std::string &ext)
{
    if (!mesh_valid_) throw std::invalid_argument("saveMesh: no isosurface has been extracted");
    if (ext != "stl" && ext != "ply") throw std::invalid_argument("saveMesh: the extension must be \"stl\" or \"ply\"");
    std::vector<float> pos((size_t)mesh_nv_ * 3), nrm((size_t)mesh_nv_ * 3);
    std::vector<uint32_t> tri((size_t)mesh_nt_ * 3);
    readMesh(pos.data(), ext == "ply" ? nrm.data() : nullptr, tri.data(), mesh_nv_, mesh_nt_);
    FILE *f = std::fopen(fn.c_str(), "wb");
    if (!f) throw IoError("saveMesh: cannot open " + fn);
    bool ok = true;
    auto put = [&](const void *p, size_t n) { ok = ok && (n == 0 || std::fwrite(p, 1, n, f) == n); };
    if (ext == "stl") {
        char header[80] = "binary STL written by vr_save_mesh";
        const uint32_t count = (uint32_t)mesh_nt_;
        put(header, sizeof(header));
        put(&count, 4);
        for (uint64_t t = 0; t < mesh_nt_ && ok; t++) {
            const float *p0 = &pos[3 * (size_t)tri[3 * t]], *p1 = &pos[3 * (size_t)tri[3 * t + 1]], *p2 = &pos[3 * (size_t)tri[3 * t + 2]];
            const double u[3] = {(double)p1[0] - p0[0], (double)p1[1] - p0[1], (double)p1[2] - p0[2]};
            const double v[3] = {(double)p2[0] - p0[0], (double)p2[1] - p0[1], (double)p2[2] - p0[2]};
            const double c[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
            const double len = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
            float rec[12] = {};
            if (len > 0.0) for (int a = 0; a < 3; a++) rec[a] = (float)(c[a] / len);
            for (int a = 0; a < 3; a++) { rec[3 + a] = p0[a]; rec[6 + a] = p1[a]; rec[9 + a] = p2[a]; }
            const uint16_t attribute = 0;
            put(rec, sizeof(rec));
            put(&attribute, 2);
        }
    } else {
        const std::string header = "ply\nformat binary_little_endian 1.0\ncomment isosurface at " + std::to_string(mesh_iso_) +
                                   ", written by vr_save_mesh\nelement vertex " + std::to_string(mesh_nv_) +
                                   "\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\n"
                                   "element face " + std::to_string(mesh_nt_) + "\nproperty list uchar uint vertex_indices\nend_header\n";
        put(header.data(), header.size());
        for (uint64_t v = 0; v < mesh_nv_ && ok; v++) {
            put(&pos[3 * (size_t)v], 12);
            put(&nrm[3 * (size_t)v], 12);
        }
        const uint8_t three = 3;
        for (uint64_t t = 0; t < mesh_nt_ && ok; t++) {
            put(&three, 1);
            put(&tri[3 * (size_t)t], 12);
        }
    }
    if (std::fclose(f) != 0) ok = false;
    if (!ok) throw IoError("saveMesh: writing " + fn + " failed");
}

// ---------------------------------------------------------------- components (vr_label_components)
void RendererCore::freeComponents()
{
    d_labels_.reset();
    comp_voxels_.clear(); comp_first_.clear(); comp_bbox_.clear(); comp_selected_.clear();
    comp_inside_ = 0;
    comp_valid_ = false;
}

void RendererCore::setComponentIndexBits(int bits)
{
    if (bits != 0 && bits != 32 && bits != 64) throw std::invalid_argument("setComponentIndexBits: 0, 32 or 64");
    comp_index_bits_ = bits;
}

// Tile pass, seam pass, flatten, the scan of the root counts; then -- the number of components known -- the labels and the
// records.  Everything new lives in locals until the very end: a call that throws leaves the previous labelling as it was.
void RendererCore::labelComponents(int32_t iso, uint64_t *n_components)
{
    requireDevice("labelComponents");
    if (!d_vol_) throw std::runtime_error("labelComponents: no dataset loaded");
    ComponentsJob J = {};
    J.volume = d_vol_.get(); J.bytes_per_voxel = res_bytes_; J.layout = vol_layout_;
    J.nx = res_dims_[0]; J.ny = res_dims_[1]; J.nz = res_dims_[2];
    J.iso_s = (float)((int64_t)iso + (datasize_bytes == 2 && (quirks & kQuirkU16Offset) ? 1000 : 0));   // isoStored's rule
    const uint64_t nvox = component_voxels(J), words = component_words(J);
    const bool fits32 = nvox < 0xffffffffull;
    if (comp_index_bits_ == 32 && !fits32) throw std::invalid_argument("labelComponents: 32-bit parents cannot number this volume's voxels");
    J.index_bits = comp_index_bits_ ? comp_index_bits_ : (fits32 ? 32 : 64);
    DeviceBuffer<uint32_t> labels, error;
    DeviceBuffer<uint64_t> parent64, bits, scan;
    DeviceBuffer<uint8_t> temp;
    const size_t temp_bytes = mesh_scan_temp_bytes(words + 1);
    labels.allocOrNoMemory(nvox, "labelComponents: hipMalloc(labels)");
    if (J.index_bits == 64) parent64.allocOrNoMemory(nvox, "labelComponents: hipMalloc(parents)");
    bits.allocOrNoMemory(words, "labelComponents: hipMalloc(root bits)");
    scan.allocOrNoMemory(words + 1, "labelComponents: hipMalloc(root counts)");
    temp.allocOrNoMemory(temp_bytes ? temp_bytes : 16, "labelComponents: hipMalloc(scan scratch)");
    error.allocOrNoMemory(1, "labelComponents: hipMalloc(error word)");
    J.labels = labels.get();
    J.parent = J.index_bits == 64 ? (void *)parent64.get() : (void *)labels.get();
    J.bits = bits.get(); J.scan = scan.get(); J.error = error.get();
    float ms = 0.0f;
    hipError_t e = hipMemsetAsync(J.error, 0, sizeof(uint32_t), stream());
    if (e == hipSuccess) e = hipEventRecord(ev0_, stream());
    if (e == hipSuccess) e = launch_components_tiles(J, stream());
    if (e == hipSuccess) e = launch_components_seams(J, stream());
    if (e == hipSuccess) e = launch_components_flatten(J, stream());
    if (e == hipSuccess) e = launch_mesh_scan(J.scan, words + 1, temp.get(), temp_bytes, stream());
    check(finishTimed(e, ms), "component kernels (union-find)");
    auto kernelsOk = [&] {
        uint32_t flags = 0;
        check(hipMemcpy(&flags, J.error, sizeof(flags), hipMemcpyDeviceToHost), "hipMemcpy(D2H error word)");
        if (flags) throw HipError(hipErrorUnknown, "labelComponents: a union-find loop hit its iteration cap (flags " + std::to_string(flags) + ")");
    };
    kernelsOk();
    uint64_t n = 0;
    check(hipMemcpy(&n, J.scan + words, sizeof(n), hipMemcpyDeviceToHost), "hipMemcpy(D2H component count)");
    if (n > 0xfffffffeull) {
        setMessage("Error!", "The volume has " + std::to_string(n) + " connected components at this iso value: more than 32-bit labels number. "
                                 "Smooth the volume or choose another iso value.");
        throw std::invalid_argument("labelComponents: more than 2^32 - 2 components");
    }
    DeviceBuffer<uint64_t> voxels, first;
    DeviceBuffer<int32_t> bbox;
    std::vector<uint64_t> h_voxels((size_t)n), h_first((size_t)n);
    std::vector<int32_t> h_bbox((size_t)n * 6);
    if (n > 0) {
        voxels.allocOrNoMemory(n, "labelComponents: hipMalloc(voxel counts)");
        first.allocOrNoMemory(n, "labelComponents: hipMalloc(first voxels)");
        bbox.allocOrNoMemory(n * 6, "labelComponents: hipMalloc(boxes)");
        J.voxels = voxels.get(); J.first_voxel = first.get(); J.bbox = bbox.get();
    }
    e = hipEventRecord(ev0_, stream());
    if (e == hipSuccess) e = launch_components_labels(J, n, stream());
    if (e == hipSuccess && n > 0) e = launch_components_records(J, stream());
    check(finishTimed(e, ms), "component kernels (labels)");
    kernelsOk();
    if (n > 0) {
        check(hipMemcpy(h_voxels.data(), J.voxels, n * sizeof(uint64_t), hipMemcpyDeviceToHost), "hipMemcpy(D2H voxel counts)");
        check(hipMemcpy(h_first.data(), J.first_voxel, n * sizeof(uint64_t), hipMemcpyDeviceToHost), "hipMemcpy(D2H first voxels)");
        check(hipMemcpy(h_bbox.data(), J.bbox, n * 6 * sizeof(int32_t), hipMemcpyDeviceToHost), "hipMemcpy(D2H boxes)");
    }
    std::vector<uint8_t> h_selected((size_t)n, 1);
    d_labels_ = std::move(labels);
    comp_voxels_ = std::move(h_voxels); comp_first_ = std::move(h_first); comp_bbox_ = std::move(h_bbox); comp_selected_ = std::move(h_selected);
    comp_inside_ = std::accumulate(comp_voxels_.begin(), comp_voxels_.end(), (uint64_t)0);
    comp_iso_ = iso; comp_iso_s_ = J.iso_s; comp_valid_ = true;
    last_comp_ms_ = ms;
    if (n_components) *n_components = n;
}

void RendererCore::componentsInfo(int32_t *iso, uint64_t *n_components, uint64_t *n_inside, uint64_t *n_selected) const
{
    if (!comp_valid_) throw std::invalid_argument("componentsInfo: no components have been labelled");
    if (iso) *iso = comp_iso_;
    if (n_components) *n_components = comp_voxels_.size();
    if (n_inside) *n_inside = comp_inside_;
    if (n_selected) *n_selected = (uint64_t)std::count(comp_selected_.begin(), comp_selected_.end(), (uint8_t)1);
}

void RendererCore::readComponents(uint64_t *voxels, uint64_t *first_voxel, int32_t *bbox6, uint8_t *selected, uint64_t capacity) const
{
    if (!comp_valid_) throw std::invalid_argument("readComponents: no components have been labelled");
    const size_t n = comp_voxels_.size();
    if ((voxels || first_voxel || bbox6 || selected) && capacity < n) throw std::invalid_argument("readComponents: buffer too small");
    if (voxels) std::copy(comp_voxels_.begin(), comp_voxels_.end(), voxels);
    if (first_voxel) std::copy(comp_first_.begin(), comp_first_.end(), first_voxel);
    if (bbox6) std::copy(comp_bbox_.begin(), comp_bbox_.end(), bbox6);
    if (selected) std::copy(comp_selected_.begin(), comp_selected_.end(), selected);
}

void RendererCore::readLabels(uint32_t *labels, uint64_t n_voxels)
{
    if (!comp_valid_) throw std::invalid_argument("readLabels: no components have been labelled");
    if (!labels || n_voxels < d_labels_.size()) throw std::invalid_argument("readLabels: buffer too small");
    requireDevice("readLabels");
    check(hipMemcpyAsync(labels, d_labels_.get(), d_labels_.bytes(), hipMemcpyDeviceToHost, stream()), "hipMemcpy(D2H labels)");
    check(hipStreamSynchronize(stream()), "hipStreamSynchronize");
}

uint32_t RendererCore::componentAt(int i, int j, int k)
{
    if (!comp_valid_) throw std::invalid_argument("componentAt: no components have been labelled");
    if (i < 0 || j < 0 || k < 0 || i >= res_dims_[0] || j >= res_dims_[1] || k >= res_dims_[2]) throw std::invalid_argument("componentAt: the voxel lies outside the volume");
    requireDevice("componentAt");
    uint32_t label = 0;
    const uint64_t at = (uint64_t)i + (uint64_t)res_dims_[0] * ((uint64_t)j + (uint64_t)res_dims_[1] * (uint64_t)k);
    check(hipMemcpyAsync(&label, d_labels_.get() + at, sizeof(label), hipMemcpyDeviceToHost, stream()), "hipMemcpy(D2H label)");
    check(hipStreamSynchronize(stream()), "hipStreamSynchronize");
    return label;
}

uint64_t RendererCore::selectComponents(uint64_t min_voxels, uint64_t keep_largest)
{
    if (!comp_valid_) throw std::invalid_argument("selectComponents: no components have been labelled");
    const size_t n = comp_voxels_.size();
    std::vector<uint8_t> sel(n, 0);
    if (keep_largest == 0 || keep_largest >= n) {
        for (size_t c = 0; c < n; c++) sel[c] = comp_voxels_[c] >= min_voxels;
    } else {
        std::vector<uint32_t> order(n);
        std::iota(order.begin(), order.end(), 0u);
        auto before = [&](uint32_t a, uint32_t b) { return comp_voxels_[a] != comp_voxels_[b] ? comp_voxels_[a] > comp_voxels_[b] : a < b; };
        std::partial_sort(order.begin(), order.begin() + (size_t)keep_largest, order.end(), before);
        for (size_t q = 0; q < (size_t)keep_largest; q++) sel[order[q]] = comp_voxels_[order[q]] >= min_voxels;
    }
    comp_selected_ = std::move(sel);
    return (uint64_t)std::count(comp_selected_.begin(), comp_selected_.end(), (uint8_t)1);
}

uint64_t RendererCore::selectComponentList(const uint32_t *labels, uint64_t n)
{
    if (!comp_valid_) throw std::invalid_argument("selectComponentList: no components have been labelled");
    if (!labels && n > 0) throw std::invalid_argument("selectComponentList: null list");
    for (uint64_t q = 0; q < n; q++)
        if (labels[q] == 0 || labels[q] > comp_voxels_.size()) throw std::invalid_argument("selectComponentList: label " + std::to_string(labels[q]) + " does not exist");
    std::vector<uint8_t> sel(comp_voxels_.size(), 0);
    for (uint64_t q = 0; q < n; q++) sel[labels[q] - 1u] = 1;
    comp_selected_ = std::move(sel);
    return (uint64_t)std::count(comp_selected_.begin(), comp_selected_.end(), (uint8_t)1);
}

// The selection as one bit per voxel (a small kernel over the labels), then extractIsosurface's body with that plane as INSIDE
void RendererCore::extractComponents(uint64_t *n_vertices, uint64_t *n_triangles)
{
    requireDevice("extractComponents");
    if (!comp_valid_) throw std::invalid_argument("extractComponents: no components have been labelled");
    if (!d_vol_) throw std::runtime_error("extractComponents: no dataset loaded");
    const uint64_t nvox = d_labels_.size(), words = (nvox + 63) / 64;
    DeviceBuffer<uint64_t> plane;
    DeviceBuffer<uint8_t> selected;
    plane.allocOrNoMemory(words, "extractComponents: hipMalloc(selection plane)");
    float ms = 0.0f;
    hipError_t e = hipSuccess;
    if (comp_selected_.empty()) {
        e = hipMemsetAsync(plane.get(), 0, plane.bytes(), stream());
        if (e == hipSuccess) e = hipStreamSynchronize(stream());
        check(e, "hipMemset(selection plane)");
    } else {
        selected.allocOrNoMemory(comp_selected_.size(), "extractComponents: hipMalloc(selection)");
        e = hipMemcpyAsync(selected.get(), comp_selected_.data(), comp_selected_.size(), hipMemcpyHostToDevice, stream());
        if (e == hipSuccess) e = hipEventRecord(ev0_, stream());
        if (e == hipSuccess) e = launch_components_plane(d_labels_.get(), selected.get(), nvox, plane.get(), stream());
        check(finishTimed(e, ms), "selection kernel");
    }
    extractMesh(comp_iso_, comp_iso_s_, plane.get(), ms, n_vertices, n_triangles);
}

}  // namespace vr
