// vr_generic.hip -- the generic ray-march kernel: the shader line by line, every mode a run-time switch
// Part of vr_kernels.hip (textually included there, inside namespace vr, once per translation unit VR_TU): not a
// translation unit of its own.  Split out of vr_kernels.hip in round 6; the arithmetic contract is stated in that file's header.
#ifndef VR_TU_MAIN
#error "include through vr_kernels.hip"
#endif

// ------------------------------------------------------------------ generic kernel
// One kernel that follows the shader line by line and takes every mode as a run-time
// (wave-uniform) switch.  It is the correctness backbone: every configuration the
// specialised kernels do not cover runs here.
// It samples through VolumeSampler (vr_sampler.h), like the isosurface, reslice and shading kernels.
template <typename VoxelT, int LAYOUT, bool COUNT, bool BIG>
__global__ __launch_bounds__(256) void raymarch_generic_kernel(const FrameParams P, const int filter,
                                                               const int is_mip, const int divmode,
                                                               const uint32_t vol_bytes,
                                                               const VoxelT *__restrict__ vol,
                                                               const float4 *__restrict__ tf,
                                                               float4 *__restrict__ fb,
                                                               uint32_t *__restrict__ spp,
                                                               const unsigned tiles_x, const unsigned tiles_y)
{
    unsigned tx, ty;
    tile_of_block(blockIdx.x, tiles_x, tiles_y, tx, ty);
    if (tx == 0xffffffffu) return;
    int lx, ly, px, py;
    if (!tile_pixel(P, tx, ty, lx, ly, px, py)) return;

    const Ray ray = compute_ray(P, (float)px + 0.5f, (float)py + 0.5f);
    float t_min = 0.0f, t_max = 0.0f;
    float d0 = 0.0f, d1 = 0.0f, d2 = 0.0f, d3 = 0.0f;
    uint32_t fetches = 0;
    if (intersect_ray_aabb(P, ray, t_min, t_max)) {
        const VolumeSampler<VoxelT, LAYOUT, BIG> S(P, vol, vol_bytes);
        const float EPSILON = 0.000001f;
        const float sx = ray.ox + ray.dx * t_min, sy = ray.oy + ray.dy * t_min, sz = ray.oz + ray.dz * t_min;
        const float p0x = sx + ray.dx * EPSILON, p0y = sy + ray.dy * EPSILON, p0z = sz + ray.dz * EPSILON;
        const float dsx = ray.dx * P.step, dsy = ray.dy * P.step, dsz = ray.dz * P.step;
        float qx = p0x, qy = p0y, qz = p0z;
        for (int i = 0; i < P.max_steps; i++) {
            if (P.accum == 1) {
                const float fi = (float)i;
                qx = p0x + fi * dsx; qy = p0y + fi * dsy; qz = p0z + fi * dsz;
            }
            float tcx, tcy, tcz;
            texcoord(P, divmode, qx, qy, qz, tcx, tcy, tcz);
            if (tcx > 1.0f || tcy > 1.0f || tcz > 1.0f || tcx < 0.0f || tcy < 0.0f || tcz < 0.0f || d3 >= 0.95f)
                break;
            float s;
            if (filter == 0) {
                const int vi = clampi(floor_to_int_sat(tcx * P.fdim[0]), 0, P.nx - 1);
                const int vj = clampi(floor_to_int_sat(tcy * P.fdim[1]), 0, P.ny - 1);
                const int vk = clampi(floor_to_int_sat(tcz * P.fdim[2]), 0, P.nz - 1);
                s = S.voxel(vi, vj, vk);
            } else {
                s = S.trilinear(tcx * P.fdim[0] - 0.5f, tcy * P.fdim[1] - 0.5f, tcz * P.fdim[2] - 0.5f);
            }
            fetches++;
            // window (VolumeRenderer.cs:122-124; Q4: max==min defined as 0)
            s = window_map(P, s, DIV_EXACT);
            float s0 = s, s1 = s, s2 = s, s3 = s;
            if (P.tf_len > 1) {
                const int idx = tf_index(P, s);
                const float4 t = tf[idx];
                s0 = t.x; s1 = t.y; s2 = t.z; s3 = t.w;
            }
            if (is_mip == 1) {
                s0 *= P.alpha_scale; s1 *= P.alpha_scale; s2 *= P.alpha_scale; s3 *= P.alpha_scale;
                if (d3 < s3) { d0 = s0; d1 = s1; d2 = s2; d3 = s3; }
            } else {
                s3 *= P.alpha_scale;
                s0 *= s3; s1 *= s3; s2 *= s3;
                const float om = 1.0f - d3;
                d0 += s0 * om; d1 += s1 * om; d2 += s2 * om; d3 += s3 * om;
                if (d3 > 0.99f) break;
            }
            if (P.accum == 0) { qx += dsx; qy += dsy; qz += dsz; }
        }
    }
    const size_t pix = (size_t)(P.fb_compact ? ly : py) * (size_t)P.img_w + (size_t)px;
    store_pixel(P, fb, pix, d0, d1, d2, d3);
    if (COUNT) spp[pix] = fetches;
}
