// vr_iso.h -- host-callable launcher of the first-hit isosurface kernel (vr_iso.hip).
// The iso parameters travel as extra kernel arguments: FrameParams and LaunchConfig, and with them the code objects and
// kernarg layouts of the vr_kernels.hip units, are the same as without the mode.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vr_frame.h"

namespace vr {

struct IsoArgs {
    float iso_s;                 // the iso value in stored voxel units (vr_core.h: vr_set_isosurface)
    float *depth;                // device: one float per colour-target pixel, indexed like it (compact-aware)
    const uint16_t *skip_grid;   // device: the dilated per-8^3-cell maximum; nullptr = no skipping
};

// one launch of raymarch_iso_kernel for (P, L): the bytes per voxel pick the translation unit
hipError_t launch_raymarch_iso(const FrameParams &P, const LaunchConfig &L, const IsoArgs &A, const void *vol, const float4 *tf,
                               float4 *fb, uint32_t *spp, hipStream_t st, const char **kernel_name);

}  // namespace vr
