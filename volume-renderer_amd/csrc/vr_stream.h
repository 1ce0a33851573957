// vr_stream.h -- host-callable launchers of vr_stream.hip: the ray-ordered sample stream of a still view (vr_set_ray_stream)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tile_schedule.h"
#include "vr_frame.h"
#include "vr_stream_pack.h"

namespace vr {

// The stream's blocks are the 8x8-pixel wavefront tiles of the fast kernel's 32x16-pixel workgroup tiles: 4 x 2 of them per
// tile, whole tiles even where the image ends inside one (their lanes outside the image hold no sample).
constexpr unsigned kStreamGroup = 4;          // G: samples a lane reads with one load (the packed format: kStreamGroup12 = 8)
struct StreamGrid { unsigned blocks_x, blocks_y, blocks; };
inline StreamGrid streamGrid(int img_w, int rows)
{
    StreamGrid g;
    g.blocks_x = (unsigned)((img_w + (int)kFastTileW - 1) / (int)kFastTileW) * (kFastTileW / 8u);
    g.blocks_y = (unsigned)((rows + (int)kFastTileH - 1) / (int)kFastTileH) * (kFastTileH / 8u);
    g.blocks = g.blocks_x * g.blocks_y;
    return g;
}

// what a replayed frame reads (device pointers; VolumeCopies owns them)
struct RayStreamView {
    const void *samples;          // VoxelT: sample i of lane l of block b at offsets[b] + (i / G) * 64 * G + l * G + i % G
    const uint16_t *counts;       // n per pixel, blocks * 64 (lane-major inside a block)
    const uint64_t *offsets;      // blocks + 1 element offsets; the last is the stream's length
    // kStreamPack12 (16-bit volumes; vr_stream_pack.h): G = 8, a sample is voxel - base in 12 bits, group i / 8 of lane l is the
    // three dwords at byte offsets[b] * 3 / 2 + (i / 8) * 768 + l * 12
    StreamFormat format = kStreamRaw;
    int base = 0;
    int table = 0;                // the frame's choice (RendererCore: vr_set_ray_stream_table): 1 = the hybrid classification where eligible
};

// The hybrid classification of a replayed frame (vr_stream.hip: TSHARE): a fixed share of the grey ramp's samples through an
// LDS table of the window's entries.  Eligible: the grey composite without a transfer function and the plain MIP (the other
// modes classify every sample through their table already), a window of at most kStreamTableMax entries, and -- packed format --
// a window the stream's base folds into (a window beyond that bound runs the integer add and stays arithmetic).
constexpr int kStreamTableMax = 4096;         // == FAST_LUT_MAX (vr_device.h)
// The automatic rule (vr_set_ray_stream_table 1) takes the hybrid on a packed stream whose samples are larger than this (the
// last-level cache, as the packed format's own rule): the headline's 744 MB gain 10 % and the cfg2 shape's 330 MB 6 %.  Below
// it, and on the unpacked formats, the gains measured are smaller (3 % on a 122 MB u16 stream, none on 437 MB) and the
// automatic mode keeps the table-less instances (docs/lab-notebook.md)
constexpr uint64_t kStreamTableMinBytes = 256ull << 20;
inline bool streamTableEligible(const FrameParams &P, const LaunchConfig &L, const RayStreamView &S)
{
    (void)L;
    if (P.tf_len > 1 || P.tf_grey != 0) return false;
    const long long entries = (long long)P.max_val - (long long)P.min_val + 1;
    if (entries < 1 || entries > kStreamTableMax) return false;
    return S.format != kStreamPack12 || streamBaseFoldsIntoWindow(P.min_val, P.max_val, S.base);
}

// pass 1: the geometric sample count n of every ray into counts[blocks * 64] and n_max(block) * 64 -- n_max rounded up to
// `group` -- into block_elems[blocks]
hipError_t launch_stream_count(const FrameParams &P, const LaunchConfig &L, uint16_t *counts, uint32_t *block_elems, unsigned group, hipStream_t st);
// block_elems of a smaller group size rounded up to whole groups of `group` (a multiple of it), in place
hipError_t launch_stream_regroup(uint32_t *block_elems, unsigned blocks, unsigned group, hipStream_t st);
// exclusive scan of block_elems into offsets[blocks + 1] (64-bit element offsets; offsets[blocks] = the total)
hipError_t launch_stream_scan(const uint32_t *block_elems, uint64_t *offsets, unsigned blocks, hipStream_t st);
// pass 2: the raw voxel of sample i of every ray into the stream (a padded slot holds voxel (0, 0, 0)); kStreamPack12:
// voxel - base in 12 bits (a padded slot holds 0)
hipError_t launch_stream_record(const FrameParams &P, const LaunchConfig &L, const void *vol, const uint16_t *counts,
                                const uint64_t *offsets, void *samples, StreamFormat format, int base, hipStream_t st);
// a frame from the stream: classification and compositing of every recorded sample (the fast kernel's modes; needs L.tile_table)
hipError_t launch_raymarch_stream(const FrameParams &P, const LaunchConfig &L, const float4 *tf, float4 *fb, const RayStreamView &S,
                                  hipStream_t st, const char **kernel_name);

}  // namespace vr
