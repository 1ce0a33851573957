// vr_components.h -- host-callable launchers of the connected-component kernels (vr_components.hip, vr_label_components):
// union-find over the inside voxels of the resident volume under the 14-neighbourhood of the extraction's seven edge
// directions.  The definition, step by step, is in include/vr_core.h and DESIGN.md section 1.6;
// tests/components_ref/components_ref.c restates it on the CPU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vr {

// One labelling.  Voxel numbers are linear indices i + nx * (j + ny * k) whatever the volume's layout.
//   parent: one index per voxel, index_bits wide (32: uint32_t, 64: uint64_t); all ones for an outside voxel.
//   bits:   one bit per voxel in linear order, 64 to a word (component_words): the voxel is a root -- its component's first voxel.
//   scan:   component_words + 1 words: the roots of each word, scanned exclusively in place by launch_scan64; the last word
//           then holds the number of components.
//   labels: one uint32 per voxel; with 32-bit parents this may be the parent array itself (the labels replace it in place).
//   error:  one word, zeroed by the caller; a kernel ORs a kComponents* bit into it instead of looping without bound.
struct ComponentsJob {
    const void *volume;                 // allocVolume's storage
    int bytes_per_voxel, layout;
    int nx, ny, nz;
    float iso_s;                        // the iso value in stored units
    int index_bits;
    void *parent;
    uint64_t *bits, *scan;
    uint32_t *labels;
    uint32_t *error;
    // records, one entry per component (label - 1); launch_components_labels writes first_voxel and initialises the others
    uint64_t *voxels, *first_voxel;
    int32_t *bbox;                      // lo x, y, z, hi x, y, z (inclusive)
};

constexpr uint32_t kComponentsFindCap = 1u << 0;     // a find walked more links than kFindCap
constexpr uint32_t kComponentsUnionCap = 1u << 1;    // a union retried more often than kUnionCap
constexpr uint32_t kComponentsBadParent = 1u << 2;   // an inside voxel's chain reached the outside sentinel

inline uint64_t component_voxels(const ComponentsJob &J) { return (uint64_t)J.nx * (uint64_t)J.ny * (uint64_t)J.nz; }
inline uint64_t component_words(const ComponentsJob &J) { return (component_voxels(J) + 63) / 64; }

// the launches of one labelling, in this order (one stream); between flatten and labels the host scans J.scan and reads the
// number of components, which sizes the records
hipError_t launch_components_tiles(const ComponentsJob &J, hipStream_t st);     // union-find inside every 8x8x8 tile, in LDS
hipError_t launch_components_seams(const ComponentsJob &J, hipStream_t st);     // unions across the tiles' faces
hipError_t launch_components_flatten(const ComponentsJob &J, hipStream_t st);   // parent = root; root bits and their counts
hipError_t launch_components_labels(const ComponentsJob &J, uint64_t n_components, hipStream_t st);   // labels; first voxels; empty records
hipError_t launch_components_records(const ComponentsJob &J, hipStream_t st);   // voxel counts and boxes

// bit v of `plane` (component_words words) = voxel v's component is selected (selected: one byte per component)
hipError_t launch_components_plane(const uint32_t *labels, const uint8_t *selected, uint64_t n_voxels, uint64_t *plane, hipStream_t st);

}  // namespace vr
