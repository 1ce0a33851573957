// volume_copies.h -- what RendererCore builds lazily from the voxels of the volume it renders and drops with them: the optional
// speed copies (12-bit packed copy, TRILINEAR's apron copy and its two per-axis permutations), bounded by the copy budget, and
// the skip grid -- and the ray-ordered sample stream of a still view (vr_stream.hip), which also depends on the ray geometry.  WHEN each is wanted is RendererCore's policy (refreshPacked12 / refreshApron / ensureSkipGrid); this class
// allocates, runs the build kernel, synchronises, frees on error and remembers a refusal.
#pragma once
#include "device_buffer.h"
#include "vr_frame.h"
#include "vr_stream.h"

namespace vr {

// bricks per axis of the VR_LAYOUT_BRICKED storage (vr_frame.h: BRICK_X x BRICK_Y x BRICK_Z voxels)
inline uint32_t bricksX(int n) { return (uint32_t)((n + BRICK_X - 1) / BRICK_X); }
inline uint32_t bricksY(int n) { return (uint32_t)((n + BRICK_Y - 1) / BRICK_Y); }
inline uint32_t bricksZ(int n) { return (uint32_t)((n + BRICK_Z - 1) / BRICK_Z); }

// the volume the copies are built from, and the stream the build kernels run on
struct ResidentVolume { const void *data; int nx, ny, nz, bytes_per_voxel, layout, exact_min, exact_max; hipStream_t stream; };

class VolumeCopies {
public:
    static constexpr uint64_t kBudgetAuto = ~0ull, kReserveBytes = 1ull << 30;
    // the reserve rule: device bytes free right now beyond max(kReserveBytes, a tenth of the device's memory), which mandatory
    // allocations (skip grid, targets, group slots) keep; false: the device does not say
    static bool freeBeyondReserve(uint64_t &bytes);
    // each: true = resident (built now if it was not); false = refused (budget / device memory; not asked again every frame:
    // setBudget and dropAll re-arm it).  A failing build kernel throws HipError and leaves no copy.
    bool ensurePacked12(const ResidentVolume &V, size_t voxels, size_t bytes);
    bool ensureApron(const ResidentVolume &V, uint64_t bytes);
    bool ensureApronPerm(const ResidentVolume &V, uint64_t bytes);   // both per-axis copies or none
    void ensureSkipGrid(const ResidentVolume &V, size_t cells);
    // The ray-ordered sample stream of the launch (P, L): samples, per-pixel counts and block offsets.  true = valid for this
    // geometry (built now if it was not: count pass, scan, ONE blocking 8-byte read-back of the total, record pass).  false =
    // refused for THIS geometry (budget / device memory; not asked again while it stands): unlike the copies' sizes the stream's
    // depends on the view, so a refusal says nothing about the next one.  invalidateRayStream: the geometry changed -- stale at
    // once, the allocation is kept for the next build, and a refusal is forgotten.
    // The format (vr_stream_pack.h: streamFormatFor) is chosen by the build from the pack mode, the volume and the size the
    // stream has unpacked, and kept with the stream; a packed build in the automatic mode reads the total back a second time
    // (the blocks are regrouped from 4 to 8 samples).  A new pack mode makes the stream stale like a new geometry.
    bool ensureRayStream(const ResidentVolume &V, const FrameParams &P, const LaunchConfig &L);
    void invalidateRayStream() { stream_valid_ = false; stream_failed_ = false; }
    void setRayStreamPack(int mode) { if (mode != stream_pack_mode_) invalidateRayStream(); stream_pack_mode_ = mode; }
    int rayStreamPack() const { return stream_pack_mode_; }
    bool rayStreamValid() const { return stream_valid_; }
    RayStreamView rayStream() const { return {stream_samples_.get(), stream_counts_.get(), stream_offsets_.get(), stream_format_, stream_base_}; }
    StreamFormat rayStreamFormat() const { return stream_valid_ ? stream_format_ : kStreamRaw; }
    uint64_t rayStreamBytes() const { return stream_valid_ ? rayStreamAllocated() : 0; }   // what a replayed frame holds resident
    uint64_t rayStreamElements() const { return stream_valid_ ? stream_elements_ : 0; }    // samples incl. padding
    uint64_t rayStreamBuilds() const { return stream_builds_; }
    void dropAll();
    void setBudget(uint64_t bytes) { budget_ = bytes; rearm(); }   // a new budget re-arms what an old one refused; frees nothing
    void trimToBudget(hipStream_t stream);   // over the budget: drop copies, the least valuable first (per-axis aprons, apron, packed copy)
    uint64_t budget() const { return budget_; }
    uint64_t copiesBytes() const { return vol12_.bytes() + apron_.bytes() + apron_perm_[0].bytes() + apron_perm_[1].bytes() + rayStreamAllocated(); }   // optional copies resident now
    bool copyFits(uint64_t bytes) const;     // may another optional copy of `bytes` be allocated (budget / free device memory)?
    const void *packed12() const { return vol12_.get(); }
    size_t packed12Bytes() const { return vol12_.bytes() - 16; }   // (every copy ends in 16 zeroed bytes of slack)
    int packed12Base() const { return vol12_base_; }                // the packed copy holds voxel - base (the dataset minimum when it was built)
    const void *apron() const { return apron_.get(); }
    size_t apronBytes() const { return apron_.bytes() - 16; }
    bool hasApronPerm() const { return apron_perm_[0] && apron_perm_[1]; }
    const void *apronPerm(int o) const { return apron_perm_[o].get(); }   // the bricks' planes along y (0) / x (1) slowest
    const uint16_t *skipGrid() const { return skip_grid_.get(); }
    uint64_t skipGridBytes() const { return skip_grid_.bytes(); }
    unsigned skipGridMin() const { return skip_grid_min_; }         // smallest cell value of the grid (read back once when it is built)

private:
    void rearm() { vol12_failed_ = apron_failed_ = apron_perm_failed_ = stream_failed_ = false; }
    uint64_t rayStreamAllocated() const { return stream_samples_.bytes() + stream_counts_.bytes() + stream_offsets_.bytes(); }
    void dropRayStream() { stream_samples_.reset(); stream_counts_.reset(); stream_offsets_.reset(); stream_valid_ = false; stream_elements_ = 0; }
    bool buildApron(const ResidentVolume &V, DeviceBuffer<uint8_t> &d, uint64_t bytes, int order);
    DeviceBuffer<uint8_t> vol12_, apron_, apron_perm_[2];
    bool vol12_failed_ = false, apron_failed_ = false, apron_perm_failed_ = false;   // refused for this volume and budget: do not retry
    int vol12_base_ = 0;
    uint64_t budget_ = kBudgetAuto;
    DeviceBuffer<uint16_t> skip_grid_;       // dilated cell-max grid
    unsigned skip_grid_min_ = 0;
    DeviceBuffer<uint8_t> stream_samples_;   // the ray-ordered sample stream (+ 16 bytes of slack)
    DeviceBuffer<uint16_t> stream_counts_;
    DeviceBuffer<uint64_t> stream_offsets_;
    bool stream_valid_ = false, stream_failed_ = false;   // failed: refused for this geometry, volume and budget
    uint64_t stream_elements_ = 0, stream_builds_ = 0;
    int stream_pack_mode_ = 1;               // vr_set_ray_stream_pack: 0 never, 1 automatic, 2 whenever lossless
    StreamFormat stream_format_ = kStreamRaw;   // of the valid stream, with the base its packed samples are relative to
    int stream_base_ = 0;
};

}  // namespace vr
