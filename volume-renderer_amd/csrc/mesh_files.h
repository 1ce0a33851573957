// mesh_files.h -- the mesh file formats of vr_save_mesh, written from host arrays.  No HIP: tests/component_records checks them with g++.
#pragma once
#include <stdint.h>

#include <stdexcept>
#include <string>

namespace vr {

struct IoError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

// Binary STL: the facet normal the unit cross product of the stored positions in double, (0, 0, 0) for a zero-area triangle,
// attribute word 0.  A file that cannot be opened or written: IoError.
void write_stl(const std::string &fn, const float *positions, const uint32_t *triangles, uint64_t nt);
// PLY, binary_little_endian 1.0: x y z nx ny nz as float, faces uchar uint
void write_ply(const std::string &fn, int32_t iso, const float *positions, const float *normals, uint64_t nv, const uint32_t *triangles, uint64_t nt);

}  // namespace vr
