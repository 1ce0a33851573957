// tile_tables.h -- the device-resident block -> tile tables of a handle (tile_schedule.h): the 32x16-pixel table every
// specialised kernel walks and the staged TRILINEAR kernel's 16x32- and 16x16-pixel ones, cached until the image, the shard,
// the camera or the skipping threshold has changed enough (tile_schedule.h: tileTablesStale).  Tables are grown, never shrunk.
#pragma once
#include <hip/hip_runtime.h>

#include "device_buffer.h"
#include "tile_schedule.h"

namespace vr {

class TileTables {
public:
    // brings the tables up to date for a launch of `rows` local rows and writes their pointers into L (the tall / small one only
    // when needed and not empty).  skip_grid: order by the tiles' visible work on this grid at P.skip_thresh (exact_max: the
    // resident volume's largest voxel); nullptr: by the geometric ray lengths.  A rebuild synchronises the stream
    void refresh(const FrameParams &P, LaunchConfig &L, int rows, bool need_tall, bool need_small, const uint16_t *skip_grid, int exact_max, hipStream_t st);
    void invalidateSkipOrder() { if (built_.skip_sig != 0) built_.skip_sig = -1; }   // an order built on another volume's visibility
    size_t bytes() const { return d_table_.bytes() + d_tall_.bytes() + d_small_.bytes() + d_work_.bytes(); }
    unsigned active() const { return active_; }   // tiles with work in the cached schedule
    double longest() const { return longest_; }   // expected samples of its longest ray

private:
    DeviceBuffer<uint32_t> d_table_, d_tall_, d_small_;   // grown only: *_blocks_ words of each are in use
    size_t blocks_ = 0, tall_blocks_ = 0, small_blocks_ = 0;
    DeviceBuffer<float> d_work_;             // per-tile cost estimates under skipping (scratch of a rebuild)
    TileTablesBuilt built_;
    unsigned active_ = 0;
    double longest_ = 0.0;
};

}  // namespace vr
