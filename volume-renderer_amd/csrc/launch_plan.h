// launch_plan.h -- what a ray-march launch runs, as rules: which kernel family a frame is eligible for, the first guess among
// its variants, the candidates of the measured choice (launch_tuner.h) and their encoding, the empty-space threshold and the
// skip grid's limits.  Host-only and HIP-free: pure functions of FrameParams / LaunchConfig and a few plain values, so they are
// tested without a device (tests/launch_plan).  RendererCore::prepareLaunch strings them together; the dispatcher
// (vr_kernels.hip: launch_raymarch) asks the same predicates.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "vr_frame.h"

namespace vr {

// true when (P, L) runs on the specialised NEAREST/composite/iterative kernel
bool fast_path_eligible(const FrameParams &P, const LaunchConfig &L);
// TRILINEAR in a grey mode with everything the batched trilinear kernel needs except the tile table
bool tri_path_candidate(const FrameParams &P, const LaunchConfig &L);
// TRILINEAR on the LDS-staged kernel (vr_tslab.hip): the trilinear path's preconditions with any mode (grey, MIP,
// transfer function), the bricked layout with its apron copy resident, torus tables that fit LDS; volumes beyond
// 32-bit offsets included
bool tri_slab_candidate(const FrameParams &P, const LaunchConfig &L);
// local image rows one launch covers (stripe padding included)
int launch_local_rows(const FrameParams &P);

// TRILINEAR on 16-bit volumes: whole brick layers are the first guess -- and the per-axis copies are not built -- only while the
// central ray keeps this share of its length along one volume axis: at 0.973 (a fifth of a voxel of shear per voxel) the
// per-tile layer thickness already wins, 1.33 against 1.46 ms on cfg3; at 1.0 whole layers do, 1.17 against 1.20
constexpr double kTriWholeLayerAlignment = 0.985;

// which tile tables (tile_tables.h) a launch wants.  any: it runs a kernel that walks one; tall / small: the staged TRILINEAR
// kernel's 16x32- and 16x16-pixel shapes (variant: vr_set_kernel_variant); skip_order: the order follows the tiles' visible
// work under empty-space skipping instead of the geometric ray lengths
struct TileTableNeeds { bool any, tall, small, skip_order; };
TileTableNeeds tileTableNeeds(const FrameParams &P, const LaunchConfig &L, int variant);

// the first guess of a launch that has its tile table (kernel variant 0 then measures, launchCandidates): writes L.sparse_shard,
// L.pipelined, L.short_batches and -- TRILINEAR on the staged kernel, variant 0 -- L.tri_slab.  tile_active / tile_longest:
// tiles with work in the schedule and the expected samples of its longest ray
void firstGuess(const FrameParams &P, LaunchConfig &L, int variant, unsigned tile_active, double tile_longest);
// the half-layer shapes (tri_slab 3 / 4) need both per-axis copies: a variant-0 launch without them (the allocation failed)
// falls back to the batched kernel where it can run, to whole layers otherwise.  After the apron refresh, before the measured choice
void halfLayerFallback(const FrameParams &P, LaunchConfig &L, int variant);

// the one encoding of a launch's variant as candidate bits: bit 0 relay kernel, 1 pipelined loop, 2 four-sample batches
// (NEAREST); tri_slab << 3 (TRILINEAR)
int choiceBits(const LaunchConfig &L);
void applyChoice(LaunchConfig &L, int bits);
// the candidate kernels (L as the heuristics left it; prior = choiceBits(L)) into out, the prior first, no duplicates; returns
// how many -- fewer than two: nothing to measure
constexpr int kMaxCandidates = 8;            // == LaunchTuner::kTuneCand (launch_plan.cpp asserts it)
int launchCandidates(const FrameParams &P, const LaunchConfig &L, int prior, int out[kMaxCandidates]);

// The ray-ordered sample stream (vr_stream.hip) holds the voxels the shader's loop reads; it stays valid exactly while this key
// stays the same, bit for bit: everything that determines WHICH voxel each sample of this launch reads -- the camera block, the
// image and the rows / stripes / Q1 limits of the launch, the volume's dimensions and box, the step and its cap, the view
// switches, the texcoord division, layout and voxel type -- and the generation of the resident voxels (RendererCore counts
// every writer of its volume).  NOT in the key, so that they render from the same stream: window, alpha, transfer function,
// MIP's compositing (its step is), the target's pointer / format / compactness, the packed copy, the tuner's variant bits.
struct RayGeometryKey {
    static constexpr int kWords = 57;
    uint32_t w[kWords];
    bool operator==(const RayGeometryKey &o) const;
    bool operator!=(const RayGeometryKey &o) const { return !(*this == o); }
};
RayGeometryKey rayGeometryKey(const FrameParams &P, const LaunchConfig &L, uint64_t volume_generation);
// may this launch be replayed from a stream at all: the fast kernel's frames, a tile table to walk, skipping not switched on
bool rayStreamEligible(const FrameParams &P, const LaunchConfig &L, int skip_empty_switch);
// default mode (vr_set_ray_stream 1): replay starts with this many consecutive launches of one geometry
constexpr int kRayStreamStillLaunches = 64;

// the largest stored value every sample at or below which classifies to alpha exactly 0 (composite mode; the window min_val ..
// max_val, tf_lut: 256 x RGBA or nullptr = grey ramp, P.alpha_scale); whole_run: the table's whole leading zero-alpha run must
// lie beyond it (TRILINEAR, whose values fall between the integers).  false: even the lowest value is visible
bool zeroAlphaThreshold(const FrameParams &P, int min_val, int max_val, const float *tf_lut, bool whole_run, int &thresh);

// the skip grid's cells (8x8x8 voxels) per axis and in all; false: beyond the grid's 32-bit byte offsets / 24-bit multiplies
bool skipGridCells(int nx, int ny, int nz, uint32_t cells3[3], size_t &total);
// NEAREST skips per batch of 8 samples, which must stay within +-1 cell of its middle sample
bool nearestBatchWithinCells(const FrameParams &P);

}  // namespace vr
