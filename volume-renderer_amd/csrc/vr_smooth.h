// vr_smooth.h -- host-callable launchers of the separable Gaussian smoothing kernels (vr_smooth.hip, vr_smooth_volume) and
// the one place the weights are computed.  The definition, operation by operation, is in include/vr_core.h and DESIGN.md
// section 1.4; tests/smooth_ref/smooth_ref.c restates it on the CPU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vr {

constexpr int kSmoothMaxRadius = 24;                    // ceil(3 * 8)
constexpr float kSmoothMaxSigma = 8.0f;

// vr_smooth_weights: r = ceil(3 sigma), w_t = (float)(exp(-t^2 / (2 sigma^2)) / sum), t = -r .. r, everything in double, the
// sum in increasing t.  false: sigma outside (0, 8] (or not finite) or capacity < 2r + 1; nothing is written then.
bool smooth_weights(float sigma, float *w, int capacity, int *radius);

// One pass along `axis` (0 x, 1 y, 2 z) over the output planes [z_begin, z_end) of an nx x ny x nz volume.
// A buffer is either voxels (bytes_per_voxel wide, in `layout`, the whole volume: allocVolume's storage) or fp32, x fastest,
// linear, holding the planes [z0, z0 + planes) of the volume.  Every plane a pass reads must be held by its input: the output
// planes for x and y, clamp(z - r .. z + r, 0, nz - 1) for z.
struct SmoothPass {
    const void *in;
    void *out;
    int in_float, out_float;            // 1: fp32 planes, 0: voxels
    int in_z0, in_planes;               // fp32 input only
    int out_z0, out_planes;             // fp32 output only
    int axis;
    int bytes_per_voxel, layout;
    int nx, ny, nz;
    int z_begin, z_end;
    int radius;
    const float *weights;               // host: 2 * radius + 1 floats from smooth_weights
};
hipError_t launch_smooth_pass(const SmoothPass &S, hipStream_t st);

}  // namespace vr
