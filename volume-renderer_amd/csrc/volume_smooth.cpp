// volume_smooth.cpp -- the passes of one Gaussian smoothing of the resident volume (vr_smooth_volume)
#include <algorithm>

#include "volume_ops.h"
#include "vr_smooth.h"

namespace vr {

// x, then y, then z, an axis with sigma 0 skipped.  With one pass the voxels go straight from src to dst.  With more, fp32 planes
// carry the intermediates: the whole volume's where one buffer fits the workspace bound, else z slabs -- the passes before z then
// also cover the r_z planes on either side of the slab, which the z pass reads (every plane of a slab is computed from the same
// inputs by the same operations as in one piece: the result does not depend on the slab size).  The buffers are freed before
// this returns.
void smooth_passes(const DeviceQueue &q, const ResidentVolume &V, const void *src, void *dst, const float sigma[3], uint64_t workspace_limit, float &ms)
{
    const int nx = V.nx, ny = V.ny, nz = V.nz;
    float w[3][2 * kSmoothMaxRadius + 1];
    int r[3] = {0, 0, 0}, axes[3], n = 0;
    for (int a = 0; a < 3; a++)
        if (sigma[a] > 0.0f) {
            if (!smooth_weights(sigma[a], w[a], 2 * kSmoothMaxRadius + 1, &r[a])) throw std::invalid_argument("smoothVolume: bad sigma");
            axes[n++] = a;
        }
    SmoothPass S = {};
    S.bytes_per_voxel = V.bytes_per_voxel; S.layout = V.layout;
    S.nx = nx; S.ny = ny; S.nz = nz;
    auto pass = [&](int a, const void *in, bool in_float, void *out, bool out_float, int buf_z0, int buf_planes, int z0, int z1) {
        S.in = in; S.out = out; S.in_float = in_float; S.out_float = out_float;
        S.in_z0 = S.out_z0 = buf_z0; S.in_planes = S.out_planes = buf_planes;
        S.axis = a; S.z_begin = z0; S.z_end = z1; S.radius = r[a]; S.weights = w[a];
        return launch_smooth_pass(S, q.stream);
    };
    ms = 0.0f;                                            // (lastSmoothMs: the passes, first launch to last)
    if (n == 1) {
        hipError_t e = hipEventRecord(q.ev0, q.stream);
        if (e == hipSuccess) e = pass(axes[0], src, false, dst, false, 0, 0, 0, nz);
        q.check(q.finishTimed(e, ms), "smooth kernel");
        return;
    }
    const int rz = sigma[2] > 0.0f ? r[2] : 0;           // planes either side of a slab the passes before z must cover
    const uint64_t plane_bytes = (uint64_t)nx * (uint64_t)ny * sizeof(float);
    const int nbuf = n - 1;
    uint64_t bound = workspace_limit;
    if (bound == 0) {
        bound = 2ull << 30;
        uint64_t room = 0;
        if (VolumeCopies::freeBeyondReserve(room)) bound = std::min<uint64_t>(bound, room / (uint64_t)nbuf);
    }
    uint64_t planes = std::min<uint64_t>(bound / plane_bytes, (uint64_t)nz);
    if (planes < (uint64_t)std::min(nz, 2 * rz + 1))
        throw DeviceMemoryError(hipErrorOutOfMemory, "smoothVolume: the workspace cannot hold one slab of fp32 planes");
    const int slab = planes >= (uint64_t)nz ? nz : (int)planes - 2 * rz;      // output planes per slab
    DeviceBuffer<uint8_t> buf[2];
    for (int b = 0; b < nbuf; b++) buf[b].allocOrNoMemory(planes * plane_bytes, "smoothVolume: hipMalloc(fp32 planes)");
    hipError_t e = hipEventRecord(q.ev0, q.stream);
    for (int s0 = 0; s0 < nz && e == hipSuccess; s0 += slab) {
        const int s1 = std::min(s0 + slab, nz), e0 = std::max(s0 - rz, 0), e1 = std::min(s1 + rz, nz);
        const void *in = src;
        for (int k = 0; k < n && e == hipSuccess; k++) {
            const bool last = k == n - 1;
            void *out = last ? dst : buf[k & 1].get();
            e = pass(axes[k], in, k > 0, out, !last, e0, e1 - e0, last ? s0 : e0, last ? s1 : e1);
            in = out;
        }
    }
    q.check(q.finishTimed(e, ms), "smooth kernel");
}

}  // namespace vr
