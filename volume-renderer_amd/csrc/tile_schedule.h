// tile_schedule.h -- work-ordered, XCD-balanced block -> tile table for the fast kernel.
//
// Rays that cross the whole volume take ~4x longer than rays clipping a corner, and one
// frame is only ~1.3 "rounds" of resident wavefronts, so dispatch order decides the tail:
// blocks are issued longest-first (LPT) and dealt round-robin to the 8 XCDs (block b runs
// on XCD b % 8).  A scheduling heuristic only: pixels are independent, the image does not
// depend on it.
#pragma once
#include <stdint.h>

#include <vector>

#include "vr_frame.h"

namespace vr {

constexpr unsigned kFastTileW = 32, kFastTileH = 16, kFastChunk = 4;   // kFastChunk: table-less fallback order
constexpr unsigned kFastChunkW = 1, kFastChunkH = 1;                    // chunk of tiles dealt to one XCD
constexpr uint32_t kTilePadding = 0xffffffffu;

// table[b] = tile_x | tile_y << 16 for block b, kTilePadding for padding blocks.
// `rows` = local image rows of this launch (stripe padding included).
// returns the number of tiles with a non-zero work estimate (*max_ray_samples: the longest ray's expected sample count)
// tile_h / tile_w: rows / columns per tile (kFastTileH x kFastTileW; the staged trilinear kernel also runs 32x32-pixel tiles on
// 16-wavefront workgroups and 16x32-pixel ones)
// work_scale (tiles_x * tiles_y floats in (0, 1], row-major; nullptr = none): the ORDER follows the geometric ray lengths times
// these -- empty-space skipping, where a tile's cost is its rays' visible stretch (vr_kernels.hip: tile_visible_work_kernel)
unsigned buildTileSchedule(const FrameParams &P, int rows, std::vector<uint32_t> &table, double *max_ray_samples = nullptr, unsigned tile_h = kFastTileH,
                           unsigned tile_w = kFastTileW, const float *work_override = nullptr);

// how close the view is to a volume axis: |largest component| of the central ray's direction in voxel units, 1 = along
// an axis, 0.58 = along the space diagonal.  Launch heuristics only (RendererCore::prepareLaunch).
double viewAxisAlignment(const FrameParams &P);
// the central ray's two smaller |components| (voxel units) over its largest: 0, 0 = along an axis; 1, 1 = a body diagonal
void viewAxisRatios(const FrameParams &P, double &mid_over_max, double &min_over_max);

// cheap fingerprint of everything the schedule depends on; with_camera = false: of everything
// that decides WHICH tiles exist (image, shard, volume box) -- the camera only decides their order
uint64_t tileScheduleKey(const FrameParams &P, int rows, bool with_camera = true);

// ---- when cached tables (tile_tables.h) are built again
// what an order under empty-space skipping was built for, in 32nds of the data's range: a window slider dragged under skipping
// would otherwise rebuild the table -- host sort, device estimate, two synchronisations -- on every frame; the order is a
// heuristic and changes gradually with the threshold.  Never 0, which stands for the geometric order
int64_t skipOrderSignature(int skip_thresh, int exact_max);
// what the cached tables were built for
struct TileTablesBuilt {
    bool table = false, tall = false, small = false;   // which tables hold blocks
    uint64_t shape_key = 0;                  // tileScheduleKey(P, rows, false)
    int64_t skip_sig = 0;                    // 0 = geometric ray lengths, skipOrderSignature() = visible work (-1: rebuild)
    float cam[21] = {};                      // the camera block of the cached order
};
// The tables must list exactly the tiles of this image / shard (shape key); the camera only decides their ORDER, a speed
// heuristic.  While the camera moves (GUI orbit: every frame) the cached order is kept until the camera block has drifted
// noticeably, so that the host-side rebuild + upload (~0.7 ms at 1080p) is not paid per frame.
bool tileTablesStale(const TileTablesBuilt &built, uint64_t shape_key, const float cam[21], int64_t skip_sig, bool need_tall, bool need_small);

}  // namespace vr
