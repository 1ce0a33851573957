// volume_copies.h -- what RendererCore builds lazily from the voxels of the volume it renders and drops with them: the optional
// speed copies (12-bit packed copy, TRILINEAR's apron copy and its two per-axis permutations), bounded by the copy budget, and
// the skip grid.  WHEN each is wanted is RendererCore's policy (refreshPacked12 / refreshApron / ensureSkipGrid); this class
// allocates, runs the build kernel, synchronises, frees on error and remembers a refusal.
#pragma once
#include "device_buffer.h"
#include "vr_frame.h"

namespace vr {

// bricks per axis of the VR_LAYOUT_BRICKED storage (vr_frame.h: BRICK_X x BRICK_Y x BRICK_Z voxels)
inline uint32_t bricksX(int n) { return (uint32_t)((n + BRICK_X - 1) / BRICK_X); }
inline uint32_t bricksY(int n) { return (uint32_t)((n + BRICK_Y - 1) / BRICK_Y); }
inline uint32_t bricksZ(int n) { return (uint32_t)((n + BRICK_Z - 1) / BRICK_Z); }

// the volume the copies are built from, and the stream the build kernels run on
struct ResidentVolume { const void *data; int nx, ny, nz, bytes_per_voxel, layout, exact_min; hipStream_t stream; };

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
    void dropAll();
    void setBudget(uint64_t bytes) { budget_ = bytes; rearm(); }   // a new budget re-arms what an old one refused; frees nothing
    void trimToBudget(hipStream_t stream);   // over the budget: drop copies, the least valuable first (per-axis aprons, apron, packed copy)
    uint64_t budget() const { return budget_; }
    uint64_t copiesBytes() const { return vol12_.bytes() + apron_.bytes() + apron_perm_[0].bytes() + apron_perm_[1].bytes(); }   // optional copies resident now
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
    void rearm() { vol12_failed_ = apron_failed_ = apron_perm_failed_ = false; }
    bool buildApron(const ResidentVolume &V, DeviceBuffer<uint8_t> &d, uint64_t bytes, int order);
    DeviceBuffer<uint8_t> vol12_, apron_, apron_perm_[2];
    bool vol12_failed_ = false, apron_failed_ = false, apron_perm_failed_ = false;   // refused for this volume and budget: do not retry
    int vol12_base_ = 0;
    uint64_t budget_ = kBudgetAuto;
    DeviceBuffer<uint16_t> skip_grid_;       // dilated cell-max grid
    unsigned skip_grid_min_ = 0;
};

}  // namespace vr
