// vr_march.h -- what the first-hit isosurface kernel (vr_iso.hip) and the gradient-lit composite kernel (vr_shade.hip) wrap
// around the shared sampler (vr_sampler.h) and compile to the same code from one definition: NEAREST's voxel index, the ray's first
// position and step, TRILINEAR's lower tap and the skip cell of a sample.  Arithmetic contract as in vr_kernels.hip.
#pragma once
#include "vr_sampler.h"

namespace vr {

// NEAREST: the voxel of a texture coordinate along one axis
__device__ __forceinline__ int nearest_index(float tc, float fdim, int n) { return clampi(floor_to_int_sat(tc * fdim), 0, n - 1); }

// the composite mode's ray: p0 = (o + dir * t_min) + dir * EPSILON, ds = dir * step
struct RayStart { float p0x, p0y, p0z, dsx, dsy, dsz; };
__device__ __forceinline__ RayStart ray_start(const FrameParams &P, const Ray &ray, float t_min)
{
    const float EPSILON = 0.000001f;
    const float sx = ray.ox + ray.dx * t_min, sy = ray.oy + ray.dy * t_min, sz = ray.oz + ray.dz * t_min;
    return RayStart{sx + ray.dx * EPSILON, sy + ray.dy * EPSILON, sz + ray.dz * EPSILON, ray.dx * P.step, ray.dy * P.step, ray.dz * P.step};
}

// the lower tap of a TRILINEAR sample along one axis, clamped: the voxel its skip cell is taken from
__device__ __forceinline__ int lower_tap(float u, int n) { return clampi((int)floorf(u), 0, n - 1); }

// Empty-space skipping per 8^3 cell: the cell of voxel (vi, vj, vk), and the grid read only when the ray enters another cell.
// is_empty(dilated cell maximum) is the mode's own test.
struct SkipCell {
    uint32_t cell = 0xffffffffu;
    bool empty = false;
    template <class IsEmpty>
    __device__ __forceinline__ bool enter(const FrameParams &P, const uint16_t *__restrict__ grid, int vi, int vj, int vk, IsEmpty is_empty)
    {
        const uint32_t c = ((uint32_t)vi >> 3) + (uint32_t)P.cnx * (((uint32_t)vj >> 3) + (uint32_t)P.cny * ((uint32_t)vk >> 3));
        if (c != cell) {
            cell = c;
            empty = is_empty(grid[c]);
        }
        return empty;
    }
};

// The central-difference gradient, its map to box axes, the normal and the headlight dot stay inline in both kernels: through a
// helper each of them changes the compiled kernels (docs/lab-notebook.md, "One code-unit scaffold ..."), and that form was not timed.

}  // namespace vr
