// vr_reslice.h -- host-callable launcher of the multi-planar reslice kernel (vr_reslice.hip).
// The plane, the slab and the values target travel as extra kernel arguments: FrameParams and LaunchConfig, and with them
// the code objects and kernarg layouts of the vr_kernels.hip units, are the same as without the mode.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vr_frame.h"

namespace vr {

// the plane in voxel index coordinates (vr_core.h: vr_set_reslice): o = centre of pixel (0, 0), du / dv = one pixel along
// x / y, dw = one slab step
struct ResliceGeom {
    float o[3], du[3], dv[3], dw[3];
};

struct ResliceArgs {
    ResliceGeom g;
    int mode;                    // VR_SLAB_MIP | VR_SLAB_MINIP | VR_SLAB_MEAN
    int n;                       // slab samples, 1 .. 1024
    int hu_offset;               // 1: the values target holds value - 1000 (16-bit data under VR_QUIRK_U16_OFFSET)
    float *values;               // device: one float per colour-target pixel, indexed like it (compact-aware)
};

// one launch of reslice_kernel for (P, L): the bytes per voxel pick the translation unit
hipError_t launch_reslice(const FrameParams &P, const LaunchConfig &L, const ResliceArgs &A, const void *vol, const float4 *tf,
                          float4 *fb, uint32_t *spp, hipStream_t st, const char **kernel_name);

}  // namespace vr
