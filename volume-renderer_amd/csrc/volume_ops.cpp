// volume_ops.cpp -- RendererCore's members for what is computed on the resident volume and the resident mesh outside a frame:
// each validates its arguments, calls the algorithm (volume_ops.h) with a queue and plain inputs, and adopts the result once the
// call has returned.  Gaussian smoothing, the rank filters (1.9), extraction (1.5), components (1.6), simplification (1.7),
// mesh smoothing (1.8).
#include <cmath>

#include "renderer_core.h"
#include "volume_ops.h"
#include "rank_schedule.h"
#include "vr_smooth.h"

namespace vr {

void RendererCore::smoothVolume(float sigma_x, float sigma_y, float sigma_z)
{
    const float sigma[3] = {sigma_x, sigma_y, sigma_z};
    for (float s : sigma)
        if (!std::isfinite(s) || s < 0.0f || s > kSmoothMaxSigma) throw std::invalid_argument("smoothVolume: every sigma must be finite and in [0, 8] voxels");
    requireDevice("smoothVolume");
    if (!d_vol_) throw std::runtime_error("smoothVolume: no dataset loaded");
    const int r3[3] = {rank_r_[0], rank_r_[1], rank_r_[2]};
    applyVolumeFilters("smoothVolume", rank_op_, r3, sigma);
}

void RendererCore::rankFilterVolume(int op, int rx, int ry, int rz)
{
    int r3[3] = {rx, ry, rz};
    if (!rank_arguments_ok(op, r3))
        throw std::invalid_argument("rankFilterVolume: op must be in 0 .. 5 and every radius in 0 .. 8 voxels (0 .. 1 for the median)");
    requireDevice("rankFilterVolume");
    if (!d_vol_) throw std::runtime_error("rankFilterVolume: no dataset loaded");
    if (rank_is_identity(op, r3)) { op = kRankOff; r3[0] = r3[1] = r3[2] = 0; }
    applyVolumeFilters("rankFilterVolume", op, r3, smooth_sigma_);
}

// G(R(loaded)) for the new state: R = (op, r3), already normalised to (OFF, 0, 0, 0) where it is the identity, G = sigma.
void RendererCore::applyVolumeFilters(const char *who, int op, const int r3[3], const float sigma[3])
{
    check(hipStreamSynchronize(stream()), "hipStreamSynchronize");      // frames in flight read the buffers replaced below
    const bool smooth = sigma[0] != 0.0f || sigma[1] != 0.0f || sigma[2] != 0.0f, rank = op != kRankOff;
    const bool off = !smooth && !rank;
    if (off && !d_loaded_) return;                                       // rendering the loaded volume already
    // The volume to render next: the loaded one again, or a new buffer the passes fill (freed with `next` if they throw, which waits
    // for them).  It is swapped in first and swapped back if the range scan fails, so a call that throws leaves the handle as it was.
    DeviceBuffer<uint8_t> next;
    if (!off) {
        DeviceBuffer<uint8_t> ranked;                                    // R's voxels where G follows; freed when the passes are done
        try {
            next = allocVolumeBuffer(res_dims_[0], res_dims_[1], res_dims_[2], res_bytes_, vol_layout_);
            if (rank && smooth) ranked = allocVolumeBuffer(res_dims_[0], res_dims_[1], res_dims_[2], res_bytes_, vol_layout_);
        } catch (const HipError &err) {
            (void)hipGetLastError();
            throw DeviceMemoryError(err.code, std::string(who) + ": " + err.what());
        }
        const void *src = d_loaded_ ? d_loaded_.get() : d_vol_.get();
        if (rank) {
            rank_passes(queue(), residentVolume(), src, smooth ? ranked.get() : next.get(), op, r3, last_rank_ms_);
            src = ranked.get();
        }
        if (smooth) smooth_passes(queue(), residentVolume(), src, next.get(), sigma, smooth_workspace_limit, last_smooth_ms_);
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
    if (off) d_loaded_.reset();                                          // the filtered volume
    else if (!d_loaded_) d_loaded_ = std::move(next);                    // (else `next` frees the earlier result)
    for (int a = 0; a < 3; a++) { smooth_sigma_[a] = sigma[a]; rank_r_[a] = r3[a]; }
    rank_op_ = op;
    dropDerived();                                                       // what a load leaves behind for new voxels
    freeComponents();                                                    // a labelling of the voxels rendered until now
}

// ---------------------------------------------------------------- the mesh (DESIGN.md sections 1.5, 1.7, 1.8)
void RendererCore::freeMesh() { mesh_.clear(); }

void RendererCore::extractIsosurface(int32_t iso, uint64_t *n_vertices, uint64_t *n_triangles)
{
    requireDevice("extractIsosurface");
    if (!d_vol_) throw std::runtime_error("extractIsosurface: no dataset loaded");
    extractMesh(iso, storedIso(iso), nullptr, 0.0f, n_vertices, n_triangles);
}

void RendererCore::extractMesh(int32_t iso, float iso_s, const uint64_t *selected, float ms, uint64_t *n_vertices, uint64_t *n_triangles)
{
    mesh_ = queueingRefusals([&] { return extract_mesh(queue(), residentVolume(), voxel_size, mesh_workspace_limit, iso, iso_s, selected, ms); });
    last_mesh_ms_ = ms;
    if (n_vertices) *n_vertices = mesh_.nv;
    if (n_triangles) *n_triangles = mesh_.nt;
}

void RendererCore::simplifyMesh(float cell, uint64_t *n_vertices, uint64_t *n_triangles)
{
    requireDevice("simplifyMesh");
    if (!std::isnormal(cell) || !(cell > 0.0f)) throw std::invalid_argument("simplifyMesh: cell must be a finite, normal number above 0");
    if (!mesh_.valid) throw std::invalid_argument("simplifyMesh: no isosurface has been extracted");
    float ms = 0.0f;
    mesh_ = queueingRefusals([&] { return simplify_mesh(queue(), mesh_, cell, ms); });
    last_simplify_ms_ = ms;
    if (n_vertices) *n_vertices = mesh_.nv;
    if (n_triangles) *n_triangles = mesh_.nt;
}

void RendererCore::meshSimplification(float *cell, uint64_t *source_vertices, uint64_t *source_triangles) const
{
    if (!mesh_.valid) throw std::invalid_argument("meshSimplification: no isosurface has been extracted");
    if (cell) *cell = mesh_.cell;
    if (source_vertices) *source_vertices = mesh_.src_nv;
    if (source_triangles) *source_triangles = mesh_.src_nt;
}

void RendererCore::smoothMesh(int iterations, float lambda, float mu, int fix_boundary)
{
    requireDevice("smoothMesh");
    if (iterations < 0 || iterations > 1000) throw std::invalid_argument("smoothMesh: iterations must be in [0, 1000]");
    if (!std::isfinite(lambda) || !(lambda > 0.0f && lambda <= 1.0f)) throw std::invalid_argument("smoothMesh: lambda must be in (0, 1]");
    if (!std::isfinite(mu) || !(mu >= -2.0f && mu <= 0.0f)) throw std::invalid_argument("smoothMesh: mu must be in [-2, 0]");
    if (!mesh_.valid) throw std::invalid_argument("smoothMesh: no isosurface has been extracted");
    float build_ms = 0.0f, iterate_ms = 0.0f;
    SmoothedMesh s = queueingRefusals([&] { return smooth_mesh(queue(), mesh_, iterations, lambda, mu, fix_boundary, build_ms, iterate_ms); });
    mesh_.setSmoothed(std::move(s.positions), std::move(s.normals), iterations, lambda, mu, fix_boundary != 0, s.n_fixed);
    last_mesh_smooth_build_ms_ = build_ms; last_mesh_smooth_iterate_ms_ = iterate_ms;
}

void RendererCore::meshSmoothing(int *iterations, float *lambda, float *mu, int *fix_boundary, uint64_t *fixed_vertices) const
{
    if (!mesh_.valid) throw std::invalid_argument("meshSmoothing: no isosurface has been extracted");
    if (iterations) *iterations = mesh_.smooth_iterations;
    if (lambda) *lambda = mesh_.smooth_lambda;
    if (mu) *mu = mesh_.smooth_mu;
    if (fix_boundary) *fix_boundary = mesh_.smooth_fix ? 1 : 0;
    if (fixed_vertices) *fixed_vertices = mesh_.smooth_fixed;
}

void RendererCore::meshInfo(int32_t *iso, uint64_t *n_vertices, uint64_t *n_triangles) const
{
    if (!mesh_.valid) throw std::invalid_argument("meshInfo: no isosurface has been extracted");
    if (iso) *iso = mesh_.iso;
    if (n_vertices) *n_vertices = mesh_.nv;
    if (n_triangles) *n_triangles = mesh_.nt;
}

void RendererCore::readMesh(float *positions, float *normals, uint32_t *triangles, uint64_t vertex_capacity, uint64_t triangle_capacity)
{
    if (!mesh_.valid) throw std::invalid_argument("readMesh: no isosurface has been extracted");
    if (((positions || normals) && vertex_capacity < mesh_.nv) || (triangles && triangle_capacity < mesh_.nt))
        throw std::invalid_argument("readMesh: buffer too small");
    requireDevice("readMesh");
    if (positions && mesh_.nv) check(hipMemcpyAsync(positions, mesh_.positions.get(), mesh_.nv * 12, hipMemcpyDeviceToHost, stream()), "hipMemcpy(D2H positions)");
    if (normals && mesh_.nv) check(hipMemcpyAsync(normals, mesh_.normals.get(), mesh_.nv * 12, hipMemcpyDeviceToHost, stream()), "hipMemcpy(D2H normals)");
    if (triangles && mesh_.nt) check(hipMemcpyAsync(triangles, mesh_.triangles.get(), mesh_.nt * 12, hipMemcpyDeviceToHost, stream()), "hipMemcpy(D2H triangles)");
    check(hipStreamSynchronize(stream()), "hipStreamSynchronize");
}

// the read-back, then the writers of mesh_files.h
void RendererCore::saveMesh(const std::string &fn, const std::string &ext)
{
    if (!mesh_.valid) throw std::invalid_argument("saveMesh: no isosurface has been extracted");
    if (ext != "stl" && ext != "ply") throw std::invalid_argument("saveMesh: the extension must be \"stl\" or \"ply\"");
    std::vector<float> pos((size_t)mesh_.nv * 3), nrm((size_t)mesh_.nv * 3);
    std::vector<uint32_t> tri((size_t)mesh_.nt * 3);
    readMesh(pos.data(), ext == "ply" ? nrm.data() : nullptr, tri.data(), mesh_.nv, mesh_.nt);
    if (ext == "stl") write_stl(fn, pos.data(), tri.data(), mesh_.nt);
    else write_ply(fn, mesh_.iso, pos.data(), nrm.data(), mesh_.nv, tri.data(), mesh_.nt);
}

// ---------------------------------------------------------------- components (vr_label_components)
void RendererCore::freeComponents() { comp_.clear(); }

void RendererCore::setComponentIndexBits(int bits)
{
    if (bits != 0 && bits != 32 && bits != 64) throw std::invalid_argument("setComponentIndexBits: 0, 32 or 64");
    comp_index_bits_ = bits;
}

void RendererCore::labelComponents(int32_t iso, uint64_t *n_components)
{
    requireDevice("labelComponents");
    if (!d_vol_) throw std::runtime_error("labelComponents: no dataset loaded");
    float ms = 0.0f;
    comp_ = queueingRefusals([&] { return label_components(queue(), residentVolume(), iso, storedIso(iso), comp_index_bits_, ms); });
    last_comp_ms_ = ms;
    if (n_components) *n_components = comp_.records.voxels.size();
}

void RendererCore::readLabels(uint32_t *labels, uint64_t n_voxels)
{
    if (!comp_.records.valid) throw std::invalid_argument("readLabels: no components have been labelled");
    if (!labels || n_voxels < comp_.labels.size()) throw std::invalid_argument("readLabels: buffer too small");
    requireDevice("readLabels");
    check(hipMemcpyAsync(labels, comp_.labels.get(), comp_.labels.bytes(), hipMemcpyDeviceToHost, stream()), "hipMemcpy(D2H labels)");
    check(hipStreamSynchronize(stream()), "hipStreamSynchronize");
}

uint32_t RendererCore::componentAt(int i, int j, int k)
{
    if (!comp_.records.valid) throw std::invalid_argument("componentAt: no components have been labelled");
    if (i < 0 || j < 0 || k < 0 || i >= res_dims_[0] || j >= res_dims_[1] || k >= res_dims_[2]) throw std::invalid_argument("componentAt: the voxel lies outside the volume");
    requireDevice("componentAt");
    uint32_t label = 0;
    const uint64_t at = (uint64_t)i + (uint64_t)res_dims_[0] * ((uint64_t)j + (uint64_t)res_dims_[1] * (uint64_t)k);
    check(hipMemcpyAsync(&label, comp_.labels.get() + at, sizeof(label), hipMemcpyDeviceToHost, stream()), "hipMemcpy(D2H label)");
    check(hipStreamSynchronize(stream()), "hipStreamSynchronize");
    return label;
}

// The selection as one bit per voxel, then extractIsosurface's body with that plane as INSIDE
void RendererCore::extractComponents(uint64_t *n_vertices, uint64_t *n_triangles)
{
    requireDevice("extractComponents");
    if (!comp_.records.valid) throw std::invalid_argument("extractComponents: no components have been labelled");
    if (!d_vol_) throw std::runtime_error("extractComponents: no dataset loaded");
    float ms = 0.0f;
    const DeviceBuffer<uint64_t> plane = selection_plane(queue(), comp_, ms);
    extractMesh(comp_.records.iso, comp_.records.iso_s, plane.get(), ms, n_vertices, n_triangles);
}

}  // namespace vr
