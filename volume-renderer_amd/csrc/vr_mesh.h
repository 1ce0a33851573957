// vr_mesh.h -- host-callable launchers of the isosurface extraction kernels (vr_mesh.hip, vr_extract_isosurface): marching
// tetrahedra on the Kuhn split of every voxel cell.  The definition, step by step, is in include/vr_core.h and DESIGN.md
// section 1.5; tests/mesh_ref/mesh_ref.c restates it on the CPU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vr {

// One z slab of an extraction.  The slab OWNS the planes [z0, z1): it writes the vertices of their voxels and the triangles of
// their cells.  Its per-voxel arrays also cover the plane z1 where the volume has one (zs = min(z1 + 1, nz)): cells of plane
// z1 - 1 reference vertices that the voxels of plane z1 own and the next slab writes.
//   scan: (zs - z0) * nx * ny + 1 words, x fastest.  After count: low half = vertices the voxel owns (0 .. 7), high half =
//         triangles of the cell whose origin the voxel is (0 .. 12; 0 outside [z0, z1)); the last word is 0.  The host scans
//         it exclusively in place (vr_primitives.h: launch_scan64), which needs both halves' sums below 2^32: kMeshMaxSlabVoxels.
//   mask: one byte per voxel of the same planes: bit d = the voxel's edge in direction d carries a vertex.
struct MeshSlab {
    const void *volume;                 // allocVolume's storage
    int bytes_per_voxel, layout;
    int nx, ny, nz;
    float iso_s;                        // the iso value in stored units
    float spacing[3];
    int z0, z1;
    uint64_t *scan;
    uint8_t *mask;
    // emit only: the mesh and this slab's first vertex and triangle in it
    float *positions, *normals;
    uint32_t *triangles;
    uint64_t vertex_base, triangle_base;
    // vr_extract_components: one bit per voxel of the WHOLE volume in linear order (launch_components_plane), which replaces
    // s >= iso_s as the definition's INSIDE; NULL: the plain comparison
    const uint64_t *selected;
};

constexpr uint64_t kMeshMaxSlabVoxels = 1ull << 28;      // 12 triangles a cell: every partial sum stays below 2^32
constexpr uint64_t kMeshBytesPerVoxel = 9;               // scan word + mask byte

inline int mesh_scan_planes(const MeshSlab &S) { return (S.z1 + 1 < S.nz ? S.z1 + 1 : S.nz) - S.z0; }
inline uint64_t mesh_scan_words(const MeshSlab &S) { return (uint64_t)mesh_scan_planes(S) * (uint64_t)S.nx * (uint64_t)S.ny + 1; }

hipError_t launch_mesh_count(const MeshSlab &S, hipStream_t st);
hipError_t launch_mesh_emit(const MeshSlab &S, hipStream_t st);

}  // namespace vr
