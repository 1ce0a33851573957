// volume_copies.cpp -- see volume_copies.h.
#include "volume_copies.h"

#include <algorithm>

#include "vr_kernels.h"

namespace vr {

bool VolumeCopies::freeBeyondReserve(uint64_t &bytes)
{
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return false; }
    const uint64_t reserve = std::max<uint64_t>(kReserveBytes, (uint64_t)total_b / 10);
    bytes = (uint64_t)free_b > reserve ? (uint64_t)free_b - reserve : 0;
    return true;
}

bool VolumeCopies::copyFits(uint64_t bytes) const
{
    if (budget_ != kBudgetAuto) return copiesBytes() + bytes <= budget_;
    uint64_t room = 0;
    return !freeBeyondReserve(room) || room >= bytes;
}

void VolumeCopies::dropAll()
{
    for (auto *q : {&vol12_, &apron_, &apron_perm_[0], &apron_perm_[1]}) q->reset();
    skip_grid_.reset();
    dropRayStream();
    rearm();
}

void VolumeCopies::trimToBudget(hipStream_t stream)
{
    if (copiesBytes() > budget_) hipCheck(hipStreamSynchronize(stream), "hipStreamSynchronize");
    if (copiesBytes() > budget_) dropRayStream();                       // (the cheapest to build again)
    if (copiesBytes() > budget_) for (auto &q : apron_perm_) q.reset();
    if (copiesBytes() > budget_) apron_.reset();
    if (copiesBytes() > budget_) vol12_.reset();
}

bool VolumeCopies::ensurePacked12(const ResidentVolume &V, size_t voxels, size_t bytes)
{
    if (vol12_ || vol12_failed_) return bool(vol12_);
    if (!copyFits(bytes + 16) || !vol12_.tryAlloc(bytes + 16)) { vol12_failed_ = true; return false; }   // an optimisation only: render from the volume as loaded
    hipError_t e = launch_pack12(V.data, vol12_.get(), voxels, (uint32_t)V.exact_min, V.stream);
    vol12_base_ = V.exact_min;
    if (e == hipSuccess) e = hipStreamSynchronize(V.stream);
    if (e != hipSuccess) vol12_.reset();
    hipCheck(e, "pack12_kernel");
    return true;
}

// one apron copy with its zeroed 16-byte tail (order 0: the apron itself, 1 / 2: the bricks' planes along y / x slowest); false: no memory
bool VolumeCopies::buildApron(const ResidentVolume &V, DeviceBuffer<uint8_t> &d, uint64_t bytes, int order)
{
    if (!d.tryAlloc(bytes + 16)) return false;
    hipError_t e = hipMemsetAsync(d.get() + bytes, 0, 16, V.stream);
    if (e == hipSuccess)
        e = launch_relayout_apron(V.data, d.get(), V.bytes_per_voxel, (uint32_t)V.nx, (uint32_t)V.ny, (uint32_t)V.nz, V.layout,
                                  (uint32_t)bricksX(V.nx), (uint32_t)bricksY(V.ny), order, V.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(V.stream);
    if (e != hipSuccess) d.reset();
    hipCheck(e, "relayout_apron_kernel");
    return true;
}

bool VolumeCopies::ensureApron(const ResidentVolume &V, uint64_t bytes)
{
    if (apron_ || apron_failed_) return bool(apron_);
    // over the budget / too little device memory left: not an error, and not asked again every frame
    if (!copyFits(bytes + 16) || !buildApron(V, apron_, bytes, 0)) { apron_failed_ = true; return false; }
    return true;
}

bool VolumeCopies::ensureApronPerm(const ResidentVolume &V, uint64_t bytes)
{
    if (apron_perm_failed_ || hasApronPerm()) return hasApronPerm();
    if (!copyFits(2 * (bytes + 16))) apron_perm_failed_ = true;
    for (int o = 0; o < 2 && !apron_perm_failed_; o++)
        if (!apron_perm_[o] && !buildApron(V, apron_perm_[o], bytes, o + 1)) apron_perm_failed_ = true;
    if (apron_perm_failed_)                                             // one without the other is 1.25 volumes of dead memory, in the low-memory case
        for (auto &q : apron_perm_) q.reset();
    return hasApronPerm();
}

bool VolumeCopies::ensureRayStream(const ResidentVolume &V, const FrameParams &P, const LaunchConfig &L)
{
    if (stream_valid_ || stream_failed_) return stream_valid_;
    const StreamGrid g = streamGrid(P.img_w, launch_local_rows(P));
    if (g.blocks == 0) return false;
    auto refuse = [&]() { dropRayStream(); stream_failed_ = true; return false; };
    // the small arrays: n per pixel, the blocks' offsets (kept from an earlier build where they are large enough)
    const size_t n_counts = (size_t)g.blocks * 64u, n_offsets = (size_t)g.blocks + 1u;
    if (stream_counts_.size() < n_counts || stream_offsets_.size() < n_offsets) {
        dropRayStream();
        if (!copyFits(n_counts * 2u + n_offsets * 8u) || !stream_counts_.tryAlloc(n_counts) || !stream_offsets_.tryAlloc(n_offsets)) return refuse();
    }
    uint64_t total = 0;
    const int64_t span = (int64_t)V.exact_max - (int64_t)V.exact_min;
    // mode 2 (and whatever can never pack) knows its format before the count; the automatic mode on a volume that could pack
    // counts in groups of 4, learns the unpacked size and regroups to 8 if that size asks for the packed format
    const bool undecided = stream_pack_mode_ == 1 && streamFormatFor(2, V.bytes_per_voxel, span, 0) == kStreamPack12;
    StreamFormat format = undecided ? kStreamRaw : streamFormatFor(stream_pack_mode_, V.bytes_per_voxel, span, 0);
    {
        DeviceBuffer<uint32_t> block_elems;
        if (!block_elems.tryAlloc(g.blocks)) return refuse();
        auto scanTotal = [&]() {
            hipError_t e = launch_stream_scan(block_elems.get(), stream_offsets_.get(), g.blocks, V.stream);
            // the stream's length: the one blocking read-back of a build
            if (e == hipSuccess) e = hipMemcpyAsync(&total, stream_offsets_.get() + g.blocks, sizeof(total), hipMemcpyDeviceToHost, V.stream);
            if (e == hipSuccess) e = hipStreamSynchronize(V.stream);
            return e;
        };
        hipError_t e = launch_stream_count(P, L, stream_counts_.get(), block_elems.get(), streamGroupOf(format), V.stream);
        if (e == hipSuccess) e = scanTotal();
        if (e == hipSuccess && undecided) {
            format = streamFormatFor(1, V.bytes_per_voxel, span, streamSampleBytes(kStreamRaw, V.bytes_per_voxel, total));
            if (format == kStreamPack12) {
                e = launch_stream_regroup(block_elems.get(), g.blocks, streamGroupOf(format), V.stream);
                if (e == hipSuccess) e = scanTotal();
            }
        }
        if (e != hipSuccess) dropRayStream();
        hipCheck(e, "stream_record_kernel (count)");
    }
    const uint64_t bytes = streamSampleBytes(format, V.bytes_per_voxel, total) + 16u;
    if (stream_samples_.bytes() < bytes) {
        stream_samples_.reset();                                         // (before the question whether the new one fits)
        if (!copyFits(bytes) || !stream_samples_.tryAlloc(bytes)) return refuse();
    }
    hipError_t e = hipSuccess;
    if (total != 0) e = launch_stream_record(P, L, V.data, stream_counts_.get(), stream_offsets_.get(), stream_samples_.get(), format, V.exact_min, V.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(V.stream);
    if (e != hipSuccess) dropRayStream();
    hipCheck(e, "stream_record_kernel");
    stream_elements_ = total;
    stream_format_ = format;
    stream_base_ = format == kStreamPack12 ? V.exact_min : 0;
    stream_valid_ = true;
    stream_builds_++;
    return true;
}

void VolumeCopies::ensureSkipGrid(const ResidentVolume &V, size_t cells)
{
    if (skip_grid_) return;
    DeviceBuffer<uint16_t> tmp(std::max<size_t>(cells * 2, 8) / 2, "skip grid tmp");   // max(cells * 2, 8) bytes: it also holds the one-word minimum below
    skip_grid_.alloc(cells, "skip grid");
    hipError_t e = launch_build_skip_grid(V.data, V.bytes_per_voxel, (uint32_t)V.nx, (uint32_t)V.ny, (uint32_t)V.nz, V.layout,
                                          bricksX(V.nx), bricksY(V.ny), tmp.get(), skip_grid_.get(), V.stream);
    // ... and its smallest cell, into the scratch cell grid (one word), read back with the build's own synchronisation
    unsigned gmin = 0;
    if (e == hipSuccess) e = launch_min_cell(skip_grid_.get(), (uint64_t)cells, reinterpret_cast<unsigned *>(tmp.get()), V.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&gmin, tmp.get(), sizeof(gmin), hipMemcpyDeviceToHost, V.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(V.stream);
    if (e != hipSuccess) skip_grid_.reset();
    hipCheck(e, "build skip grid");
    skip_grid_min_ = gmin;
}

}  // namespace vr
