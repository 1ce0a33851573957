// volume_rank.cpp -- the passes of one rank filter of the resident volume (vr_rank_filter_volume)
#include "volume_ops.h"
#include "vr_rank.h"

namespace vr {

// What rank_schedule says, launched: the minimum and the maximum one pass per axis with a radius, the median one launch; the
// passes go from src over dst and one scratch volume to dst.  The scratch volume is voxel-typed, the volume's own size, and
// freed before this returns (its destructor waits for nothing: the stretch is finished before).
void rank_passes(const DeviceQueue &q, const ResidentVolume &V, const void *src, void *dst, int op, const int r3[3], float &ms)
{
    RankStep steps[kRankMaxSteps];
    const int n = rank_schedule(op, r3, steps);
    if (n <= 0) throw std::invalid_argument("rankFilterVolume: nothing to run");
    // (the kernels read no voxel outside the volume, so the brick padding of a scratch volume needs no zeroes)
    const uint64_t voxels = V.layout == 0 ? (uint64_t)V.nx * (uint64_t)V.ny * (uint64_t)V.nz
                                          : (uint64_t)bricksX(V.nx) * (uint64_t)bricksY(V.ny) * (uint64_t)bricksZ(V.nz) * 64u;
    DeviceBuffer<uint8_t> scratch[2];
    for (int b = 0; b < rank_scratch_buffers(steps, n); b++)
        scratch[b].allocOrNoMemory((voxels + 256) * (uint64_t)V.bytes_per_voxel, "rankFilterVolume: hipMalloc(intermediate volume)");
    auto buffer = [&](int id) -> void * {
        return id == RANK_SRC ? const_cast<void *>(src) : (id == RANK_DST ? dst : scratch[id - RANK_TMP0].get());
    };
    RankPass P = {};
    P.bytes_per_voxel = V.bytes_per_voxel; P.layout = V.layout;
    P.nx = V.nx; P.ny = V.ny; P.nz = V.nz;
    for (int a = 0; a < 3; a++) P.r3[a] = r3[a];
    ms = 0.0f;                                            // (lastRankMs: the passes, first launch to last)
    hipError_t e = hipEventRecord(q.ev0, q.stream);
    for (int k = 0; k < n && e == hipSuccess; k++) {
        P.kernel = steps[k].kernel; P.axis = steps[k].axis;
        P.in = buffer(steps[k].in); P.out = buffer(steps[k].out);
        e = launch_rank_pass(P, q.stream);
    }
    q.check(q.finishTimed(e, ms), "rank filter kernel");
}

}  // namespace vr
