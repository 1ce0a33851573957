// vr_rank.h -- host-callable launcher of the rank filter kernels (vr_rank.hip, vr_rank_filter_volume): the minimum or the
// maximum along one axis, and the median over a box of radii 0 or 1.  The definition is in include/vr_core.h and DESIGN.md
// section 1.9; tests/rank_ref/rank_ref.c restates it on the CPU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rank_schedule.h"

namespace vr {

// One step of rank_schedule over a whole nx x ny x nz volume: both buffers are voxels, bytes_per_voxel wide, in `layout`
// (allocVolume's storage), and different.  RANK_MIN / RANK_MAX: along `axis` with radius r3[axis] in 1 .. 8.  RANK_MEDIAN: the
// box of r3, every radius 0 or 1 and one of them 1.
struct RankPass {
    const void *in;
    void *out;
    int kernel;                         // RankKernel
    int axis;
    int bytes_per_voxel, layout;
    int nx, ny, nz;
    int r3[3];
};
hipError_t launch_rank_pass(const RankPass &P, hipStream_t st);

}  // namespace vr
