// launch_plan.cpp -- see launch_plan.h
#include "launch_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "launch_tuner.h"
#include "tile_schedule.h"

namespace vr {

static_assert(kMaxCandidates == LaunchTuner::kTuneCand, "launch_plan.h: kMaxCandidates");

// The specialised kernel covers NEAREST + iterative accumulation with a non-degenerate
// window whose divisions were certified and alpha_scale in [0,1]: grey-ramp composite,
// grey-ramp MIP, and composite through a transfer-function table that fits LDS.
// Everything else (TRILINEAR, closed-form accumulation, MIP + TF, ...) is generic.
bool fast_path_eligible(const FrameParams &P, const LaunchConfig &L)
{
    const bool tf = P.tf_len > 1;
    if (tf && !L.use_lut) return false;
    return !L.generic && L.filter == 0 && P.accum == 0 && P.fden > 0.0f &&
           P.max_val > P.min_val && L.divmode_win == DIV_CERT && L.divmode_tc != DIV_EXACT &&
           P.alpha_scale >= 0.0f && P.alpha_scale <= 1.0f;
}

// TRILINEAR has a batched kernel for the grey modes: same preconditions as the fast path apart
// from the filter, plus 32-bit offsets, address tables that fit LDS and a tile table
bool tri_path_candidate(const FrameParams &P, const LaunchConfig &L)
{
    return !L.generic && L.filter == 1 && P.accum == 0 && P.tf_len <= 1 && P.fden > 0.0f && P.max_val > P.min_val &&
           L.divmode_win == DIV_CERT && L.divmode_tc != DIV_EXACT && P.alpha_scale >= 0.0f && P.alpha_scale <= 1.0f &&
           !L.big_offsets && P.nx + P.ny + P.nz <= FAST_AXIS_TAB_MAX;
}

// TRILINEAR on the LDS-staged kernel (vr_tslab.hip): every mode (the 256-entry transfer-function table sits in LDS), any
// volume size (64-bit DMA addresses), the bricked layout; the apron copy must be resident (host: refreshApron)
bool tri_slab_candidate(const FrameParams &P, const LaunchConfig &L)
{
    if (L.generic || L.filter != 1 || P.accum != 0 || !(P.fden > 0.0f) || !(P.max_val > P.min_val) || L.divmode_win != DIV_CERT ||
        L.divmode_tc == DIV_EXACT || !(P.alpha_scale >= 0.0f && P.alpha_scale <= 1.0f) || L.layout != 1) return false;
    if (P.tf_len > 256) return false;
    const uint64_t bricks = (uint64_t)P.bnx * (uint64_t)P.bny * (uint64_t)P.bnz;
    if (bricks >= (1ull << 32) || (uint64_t)P.bnx * (uint64_t)P.bny >= (1ull << 24)) return false;
    return P.nx <= 32768 && P.ny <= 32768 && P.nz <= 32768;           // 16-bit brick indices in the load plan; plan and tables cover a tile's own range only
}

int launch_local_rows(const FrameParams &P)
{
    int rows;
    if (P.stripe_count > 1) {
        const int nstripes_total = (P.img_h + P.stripe_rows - 1) / P.stripe_rows;
        const int mine = (nstripes_total - P.stripe_index + P.stripe_count - 1) / P.stripe_count;
        rows = mine * P.stripe_rows;
    } else {
        rows = P.row_end - P.row_begin;
    }
    return rows;
}

TileTableNeeds tileTableNeeds(const FrameParams &P, const LaunchConfig &L, int variant)
{
    TileTableNeeds n;
    n.any = fast_path_eligible(P, L) || tri_path_candidate(P, L) || tri_slab_candidate(P, L);
    n.small = L.filter == 1 && tri_slab_candidate(P, L);              // 16x16-pixel tiles for the staged trilinear kernel's small shape (four wavefronts; any stripe height that is a multiple of 16)
    n.tall = n.small && (P.stripe_count <= 1 || P.stripe_rows % 32 == 0 || variant == 9);   // 16x32-pixel tiles for its tall shape
    // empty-space skipping: the order follows the tiles' VISIBLE work (vr_kernels.hip: tile_visible_work_kernel); it changes with
    // the threshold (window / transfer function), not only with the camera
    // (NEAREST skips per ray and batch: every pose.  The staged TRILINEAR kernel skips per tile and brick layer, and its tiles
    // that do not fit the ring skip nothing: where the view is oblique the estimate misjudges exactly the longest tiles -- the
    // off-axis pose ran 1.46 / 1.55 / 2.2 ms depending on where they landed, and still 1.15 / 1.65 from one process to the next
    // once those tiles skipped per batch -- so there the order stays the geometric one: 1.19-1.20 every time)
    n.skip_order = P.skip_empty != 0 && L.skip_grid != nullptr && (L.filter == 0 || viewAxisAlignment(P) >= 0.92);
    return n;
}

void firstGuess(const FrameParams &P, LaunchConfig &L, int variant, unsigned tile_active, double tile_longest)
{
    // Kernel choice per launch (all bit-identical; measured on cfg3 after the checked-head fix, tools/pose_sweep.py and
    // tools/shard_ms.py; `aligned` = central ray within ~23 degrees of a volume axis):
    //   * relay kernel (4 wavefronts per 8x8 tile) for launches far from filling the chip -- fewer than 256 active
    //     32x16 tiles when the view is aligned (N = 8 shard: 0.107 vs 0.142 ms), fewer than 1024 when it is oblique
    //     (its rays are longer chains with more L1 misses per step: N = 2 shards 0.31-0.36 vs 0.36-0.47 ms);
    //   * otherwise the fast kernel, with its software-pipelined batch loop unless the opacity scale says rays end
    //     early (alpha >= 0.5: the speculative batch is wasted, 0.198 vs 0.189 ms): equal at the default pose
    //     (0.454 ms), 3-14 % faster over oblique poses, 12 % at an N = 4 shard (0.163 vs 0.185 ms).
    const bool aligned = viewAxisAlignment(P) >= 0.92;
    // TRILINEAR, first guess (the work model then measures): the LDS-staged kernel (vr_tslab.hip) -- whole brick layers, two
    // workgroups per CU -- when the view is aligned with a volume axis (cfg3 default pose: every tile staged, 1.25 vs 1.93 ms on
    // the batched kernel) and for 8-bit volumes at every pose (80-byte slots: orbit poses 1.1-1.4 ms against 2.1).  A 16-bit
    // volume's oblique layers do not fit three deep (240-400 bricks of 160 B): those views take the per-axis copies and half
    // layers (round 4: orbit poses 1.43-1.62 ms against 2.9-3.4 whole-layer / 2.6-3.0 batched), on 16x32-pixel tiles with the
    // ring's rows holding their own brick ranges when the view runs near a body diagonal of the volume (1.68 ms against 3.0).
    if (variant == 0 && L.filter == 1 && tri_slab_candidate(P, L)) {
        if (std::max(P.nx, std::max(P.ny, P.nz)) <= 640 && L.tile_table_small != nullptr) {
            L.tri_slab = 6;                                              // small volumes: 16x16-pixel tiles (round 6)
        } else if (viewAxisAlignment(P) >= kTriWholeLayerAlignment || L.bytes_per_voxel == 1) {
            L.tri_slab = 1;
        } else {
            double r1, r2;
            viewAxisRatios(P, r1, r2);
            // 16x32-pixel tiles only where 32 consecutive LOCAL rows are 32 consecutive image rows: with cyclic stripes of 16
            // rows a tall tile spans two stripes stripe_count*16 rows apart, its corner-ray hull (and its load plan) is that
            // much taller, and nearly every tile would march unstaged (round-4 advisor)
            const bool tall_ok = P.stripe_count <= 1 || P.stripe_rows % 32 == 0;
            L.tri_slab = (r1 > 0.7 && r2 > 0.55 && tall_ok) ? 4 : 3;
        }
    }
    // first guess of the work model (kernel variant 0 then measures): the relay kernel pays when the launch is
    // a single under-filled round of long serial rays -- few active tiles, scaled by how long the rays are (1045 samples
    // on the configuration the 256 / 1024 were measured on; a 256^3 volume's 262-sample rays want 4x fewer tiles)
    const double len_scale = std::min(1.0, std::max(0.15, tile_longest / 1000.0));
    L.sparse_shard = ((double)tile_active < (aligned ? 256.0 : 1024.0) * len_scale) ? 1 : 0;
    if (variant == 2) L.sparse_shard = 0;                // kernel variant 2: never the relay kernel
    if (variant == 3) L.sparse_shard = 1;                // kernel variant 3: always (when the shape allows)
    L.pipelined = (variant == 0 && P.alpha_scale < 0.5f) ? 1 : 0;
    L.short_batches = (variant == 0 && P.alpha_scale >= 0.5f) ? 1 : 0;     // 0.174 vs 0.190 ms at alpha = 1 (cfg3)
    if (variant == 5) { L.pipelined = 1; L.sparse_shard = 0; }   // kernel variant 5: fast kernel, pipelined loop, never the relay
}

// (without the per-axis copies: the round-3 choice)
void halfLayerFallback(const FrameParams &P, LaunchConfig &L, int variant)
{
    if ((L.tri_slab == 3 || L.tri_slab == 4) && (L.apron_y == nullptr || L.apron_x == nullptr) && variant == 0) L.tri_slab = tri_path_candidate(P, L) ? 0 : 1;
}

int choiceBits(const LaunchConfig &L)
{
    return L.filter == 1 ? (L.tri_slab << 3) : ((L.sparse_shard ? 1 : 0) | (L.pipelined ? 2 : 0) | (L.short_batches ? 4 : 0));
}

void applyChoice(LaunchConfig &L, int c)
{
    L.sparse_shard = (c & 1) ? 1 : 0; L.pipelined = (c & 2) ? 1 : 0; L.short_batches = (c & 4) ? 1 : 0; L.tri_slab = (c >> 3) & 15;
}

int launchCandidates(const FrameParams &P, const LaunchConfig &L, int prior, int cand[kMaxCandidates])
{
    int n = 0;
    auto add = [&](int c) { for (int k = 0; k < n; k++) if (cand[k] == c) return; if (n < kMaxCandidates) cand[n++] = c; };
    if (fast_path_eligible(P, L)) {
        const bool relay_ok = !L.big_offsets && !(P.skip_empty != 0 && L.skip_grid != nullptr);
        add(prior & (relay_ok ? 7 : 6));
        add(P.alpha_scale >= 0.5f ? 4 : 2);                              // fast kernel: four-sample batches / pipelined loop
        add(0);                                                          // fast kernel, plain loop
        if (relay_ok) add(1);
    } else if (L.filter == 1 && L.apron != nullptr && tri_slab_candidate(P, L)) {
        // TRILINEAR: the LDS-staged kernel in its shapes, the batched kernel where it can run
        add(prior);
        add(1 << 3);
        add(5 << 3);                                                     // three workgroups per CU: wins where the tiles' layers fit 53 KiB
        // 16x16-pixel tiles on four wavefronts: launches whose 32x16-pixel tiles leave workgroup slots empty (two per CU).
        // TRILINEAR: the small tile shape (16x16 pixels, four wavefronts, 40 KiB) is the FIRST GUESS where a tile's brick layers are small
        // against its ring -- volumes up to 640 voxels along every axis (cfg1 shape 0.138 -> 0.118 ms, cfg2 shape 0.402 -> 0.381) -- and a
        // CANDIDATE of the measured choice everywhere: on 1024^3 volumes it loses at the default pose (u16 1.12 -> 1.22 ms) and at strongly
        // oblique ones (zenith 60 / azimuth 45: 1.55 -> 2.75), but wins over most of an orbit (u8: 0.92-1.02 against 1.01-1.11 ms at five of
        // seven poses; u16 with the per-axis copies: 1.22 / 1.31 / 1.22 against 1.36 / 1.40 / 1.31; profiles/r06_trilinear_orbit.txt) -- which
        // pose does which is exactly what the measurement is for.
        if (L.tile_table_small != nullptr) add(6 << 3);
        if (tri_path_candidate(P, L)) add(0);
        if (L.apron_y != nullptr && L.apron_x != nullptr) {
            add(3 << 3);
            if (L.tile_table_tall != nullptr) add(4 << 3);
        } else if (L.bytes_per_voxel == 1 && L.tile_table_tall != nullptr && viewAxisAlignment(P) < 0.92) {
            add(4 << 3);                                                 // 8-bit volumes, oblique views: whole layers on 16x32-pixel tiles
        }
    }
    return n;
}

bool RayGeometryKey::operator==(const RayGeometryKey &o) const { return std::memcmp(w, o.w, sizeof(w)) == 0; }

RayGeometryKey rayGeometryKey(const FrameParams &P, const LaunchConfig &L, uint64_t volume_generation)
{
    RayGeometryKey k;
    int n = 0;
    auto put = [&](const void *p, int words) { std::memcpy(k.w + n, p, sizeof(uint32_t) * (size_t)words); n += words; };
    static_assert(sizeof(float) == 4 && sizeof(int32_t) == 4, "the key is words");
    put(P.cam, 21);
    put(&P.img_w, 1); put(&P.img_h, 1);
    put(&P.row_begin, 1); put(&P.row_end, 1);
    put(&P.col_lim, 1); put(&P.row_lim, 1);
    put(&P.stripe_rows, 1); put(&P.stripe_index, 1); put(&P.stripe_count, 1);
    put(&P.nx, 1); put(&P.ny, 1); put(&P.nz, 1);
    put(P.half, 3); put(P.pmin, 3); put(P.pmax, 3); put(P.ext, 3); put(P.rext, 3);
    put(&P.step, 1);
    put(&P.max_steps, 1);
    put(&P.view_top, 1); put(&P.view_bottom, 1);
    const int32_t cfg[3] = {L.divmode_tc, L.layout, L.bytes_per_voxel};
    put(cfg, 3);
    put(&volume_generation, 2);
    if (n != RayGeometryKey::kWords) std::abort();                      // (launch_plan.h: kWords)
    return k;
}

bool rayStreamEligible(const FrameParams &P, const LaunchConfig &L, int skip_empty_switch)
{
    return fast_path_eligible(P, L) && L.tile_table != nullptr && skip_empty_switch == 0;
}

// threshold: largest voxel value whose classification is exactly zero
bool zeroAlphaThreshold(const FrameParams &P, int min_val, int max_val, const float *tf_lut, bool whole_run, int &thresh)
{
    if (P.alpha_scale == 0.0f) {
        thresh = 65535;
    } else if (tf_lut == nullptr) {
        thresh = min_val;                                // v = (clamp(t) - min)/den = 0  <=>  t <= min_val
    } else {
        int e = 0;
        const int width = max_val - min_val;
        // TRILINEAR classifies values BETWEEN the integers too: they reach every table entry up to the one of the largest tap
        // (the index is monotone in the value), so there the whole leading run of entries has to be invisible
        int zero_run = 0;
        while (zero_run < 256 && tf_lut[4 * zero_run + 3] * P.alpha_scale == 0.0f) zero_run++;
        for (; e <= width; e++) {
            const float s = (float)(min_val + e);
            const float v = (s - P.fmin) / P.fden;       // == the kernel's certified quotient
            int idx = (int)std::floor(v * 255.0f + 0.5f);
            idx = std::min(std::max(idx, 0), 255);
            if (whole_run ? idx >= zero_run : tf_lut[4 * idx + 3] * P.alpha_scale != 0.0f) break;
        }
        thresh = min_val + e - 1;                        // e == 0: even the lowest entry is visible
        if (e == 0) return false;
    }
    return true;
}

bool skipGridCells(int nx, int ny, int nz, uint32_t c[3], size_t &total)
{
    c[0] = (uint32_t)(nx + 7) / 8; c[1] = (uint32_t)(ny + 7) / 8; c[2] = (uint32_t)(nz + 7) / 8;
    total = (size_t)c[0] * c[1] * c[2];
    return !(total * 2 >= (1ull << 32) || c[0] >= (1u << 24) || (uint64_t)c[1] * c[2] >= (1u << 24));
}

bool nearestBatchWithinCells(const FrameParams &P)
{
    // bound the voxel advance per step on every voxel axis (|dir| <= 1)
    float max_delta = 0.0f;
    const bool swz = (P.view_bottom == 1 || P.view_top == 1);
    const float vdim[3] = {(float)P.nx, swz ? (float)P.nz : (float)P.ny, swz ? (float)P.ny : (float)P.nz};   // voxel axis behind each box axis
    for (int a = 0; a < 3; a++) max_delta = std::max(max_delta, P.step * vdim[a] / P.ext[a]);
    return 4.0f * max_delta + 0.6f <= 8.0f;
}

}  // namespace vr
