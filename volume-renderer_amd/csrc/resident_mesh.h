// resident_mesh.h -- the mesh a handle keeps on the device: its arrays, what made it (the iso value, a simplification, the
// smoothing on top), and the one rule they share: a mesh that adopts new arrays is unsimplified and unsmoothed until told otherwise.
#pragma once
#include <stdint.h>

#include "device_buffer.h"

namespace vr {

struct ResidentMesh {
    DeviceBuffer<float> positions, normals;  // 3 floats a vertex
    DeviceBuffer<uint32_t> triangles;        // 3 indices a triangle
    uint64_t nv = 0, nt = 0;
    int32_t iso = 0;
    bool valid = false;                      // an extraction has succeeded (its mesh may be empty) and was not freed
    float cell = 0.0f;                       // the simplification that made it (0: an extraction did) and the counts of the mesh it was given
    uint64_t src_nv = 0, src_nt = 0;
    int smooth_iterations = 0;               // the last successful smoothing on it; all 0 on a new mesh
    float smooth_lambda = 0.0f, smooth_mu = 0.0f;
    bool smooth_fix = false;
    uint64_t smooth_fixed = 0;

    uint64_t bytes() const { return positions.bytes() + normals.bytes() + triangles.bytes(); }
    void clear() { *this = ResidentMesh(); }
    // a new mesh: not simplified (its source is itself), not smoothed
    void adopt(DeviceBuffer<float> &&pos, DeviceBuffer<float> &&nrm, DeviceBuffer<uint32_t> &&tri, uint64_t n_vertices, uint64_t n_triangles, int32_t iso_value)
    {
        clear();
        positions = std::move(pos); normals = std::move(nrm); triangles = std::move(tri);
        nv = src_nv = n_vertices; nt = src_nt = n_triangles; iso = iso_value; valid = true;
    }
    void setSimplified(float cell_size, uint64_t source_vertices, uint64_t source_triangles) { cell = cell_size; src_nv = source_vertices; src_nt = source_triangles; }
    // a smoothing of this mesh: new positions and normals (both empty: they stay) for the same triangles; the simplification stands
    void setSmoothed(DeviceBuffer<float> &&pos, DeviceBuffer<float> &&nrm, int iterations, float lambda, float mu, bool fix, uint64_t fixed)
    {
        if (pos) { positions = std::move(pos); normals = std::move(nrm); }
        smooth_iterations = iterations; smooth_lambda = lambda; smooth_mu = mu; smooth_fix = fix; smooth_fixed = fixed;
    }
};

}  // namespace vr
