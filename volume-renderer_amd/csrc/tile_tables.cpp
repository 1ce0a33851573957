// tile_tables.cpp -- see tile_tables.h
#include "tile_tables.h"

#include <algorithm>
#include <cstring>
#include <vector>

#include "vr_kernels.h"

namespace vr {

// Rebuild the longest-first block order when the camera / image / shard changed.  The
// table is tiny (one word per 32x16-pixel tile) and is uploaded on the launch stream.
void TileTables::refresh(const FrameParams &P, LaunchConfig &L, int rows, bool need_tall, bool need_small, const uint16_t *skip_grid, int exact_max, hipStream_t st)
{
    const uint64_t shape_key = tileScheduleKey(P, rows, false);
    const int64_t skip_sig = skip_grid ? skipOrderSignature(P.skip_thresh, exact_max) : 0;
    if (tileTablesStale(built_, shape_key, P.cam, skip_sig, need_tall, need_small)) {
        // (one small kernel and a synchronous copy per table, only when the table is rebuilt; an empty sample costs about
        // a seventh of a sampled one in both kernel families)
        auto estimate = [&](unsigned tw, unsigned th, std::vector<float> &out) {
            const size_t n = (size_t)((P.img_w + (int)tw - 1) / (int)tw) * (size_t)((rows + (int)th - 1) / (int)th);
            d_work_.ensure(2 * n, "tile work");
            hipCheck(launch_tile_visible_work(P, skip_grid, rows, tw, th, 0.15f, L.filter == 1 ? 1 : 0, d_work_.get(), st), "tile_visible_work_kernel");
            std::vector<float> both(2 * n);
            hipCheck(hipMemcpyAsync(both.data(), d_work_.get(), 2 * n * sizeof(float), hipMemcpyDeviceToHost, st), "hipMemcpy(tile work)");
            hipCheck(hipStreamSynchronize(st), "hipStreamSynchronize");
            out.resize(n);
            for (size_t t = 0; t < n; t++) out[t] = both[2 * t + 1] > 0.0f ? std::min(both[2 * t] / both[2 * t + 1], 1.0f) : 1.0f;   // cost with skipping / without
        };
        std::vector<float> work, work_tall, work_small;
        if (skip_grid) {
            estimate(kFastTileW, kFastTileH, work);
            if (need_tall) estimate(16u, 32u, work_tall);
            if (need_small) estimate(16u, 16u, work_small);
        }
        std::vector<uint32_t> table;
        active_ = buildTileSchedule(P, rows, table, &longest_, kFastTileH, kFastTileW, skip_grid ? work.data() : nullptr);
        // synchronous copies: the tables are pageable temporaries
        hipCheck(hipStreamSynchronize(st), "hipStreamSynchronize");
        auto upload = [&](DeviceBuffer<uint32_t> &d, size_t &blocks, const std::vector<uint32_t> &t) {
            d.ensure(t.size(), "tile table");
            if (!t.empty()) hipCheck(hipMemcpy(d.get(), t.data(), t.size() * sizeof(uint32_t), hipMemcpyHostToDevice), "hipMemcpy(tile table)");
            blocks = t.size();
        };
        upload(d_table_, blocks_, table);
        tall_blocks_ = small_blocks_ = 0;
        if (need_tall) {
            (void)buildTileSchedule(P, rows, table, nullptr, 32u, 16u, skip_grid ? work_tall.data() : nullptr);
            upload(d_tall_, tall_blocks_, table);
        }
        if (need_small) {
            (void)buildTileSchedule(P, rows, table, nullptr, 16u, 16u, skip_grid ? work_small.data() : nullptr);
            upload(d_small_, small_blocks_, table);
        }
        built_.shape_key = shape_key;
        built_.skip_sig = skip_sig;
        std::memcpy(built_.cam, P.cam, sizeof(built_.cam));
        built_.table = (bool)d_table_; built_.tall = tall_blocks_ > 0; built_.small = small_blocks_ > 0;
    }
    L.tile_table = d_table_.get();
    L.tile_table_blocks = (uint32_t)blocks_;
    L.tile_table_tall = nullptr; L.tile_table_tall_blocks = 0;
    L.tile_table_small = nullptr; L.tile_table_small_blocks = 0;
    if (need_tall && tall_blocks_ > 0) { L.tile_table_tall = d_tall_.get(); L.tile_table_tall_blocks = (uint32_t)tall_blocks_; }
    if (need_small && small_blocks_ > 0) { L.tile_table_small = d_small_.get(); L.tile_table_small_blocks = (uint32_t)small_blocks_; }
}

}  // namespace vr
