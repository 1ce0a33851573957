// vr_shade.h -- host-callable launcher of the gradient-lit composite kernel (vr_shade.hip, vr_set_shading).
// The shading parameters travel as extra kernel arguments: FrameParams and LaunchConfig, and with them the code objects and
// kernarg layouts of the vr_kernels.hip units, are the same as without the mode.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vr_frame.h"

namespace vr {

struct ShadeArgs {
    float ambient, diffuse, specular;   // vr_set_shading's coefficients (finite, >= 0)
    int spec_squarings;                 // log2(shininess): spec = d^shininess by this many squarings (0: spec = d)
    const uint16_t *skip_grid;          // device: the dilated per-8^3-cell maximum; nullptr = no skipping
    int32_t skip_thresh;                // a cell whose dilated maximum is <= this classifies every sample in it to alpha 0
};

// one launch of raymarch_shade_kernel for (P, L): the bytes per voxel pick the translation unit
hipError_t launch_raymarch_shade(const FrameParams &P, const LaunchConfig &L, const ShadeArgs &A, const void *vol, const float4 *tf,
                                 float4 *fb, uint32_t *spp, hipStream_t st, const char **kernel_name);

}  // namespace vr
