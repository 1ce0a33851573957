// launch_tuner.h -- the measured work model of kernel variant 0 (vr_set_autotune): which of a configuration's candidate
// kernels a launch runs.  Host-only and HIP-free: a state machine over a key, a candidate list and millisecond timings.
// launch_plan.h enumerates the candidates; RendererCore owns the events that time them and feeds the results in
// (renderer_core.cpp: tuneChoose, tuneCollect).
//
// Every candidate kernel of a configuration renders the same bits, so the first frames of a configuration double as
// measurements -- each candidate is timed a few times, the fastest is kept until the configuration changes.
// A candidate = bit set: 1 relay kernel, 2 pipelined batch loop, 4 four-sample batches; bits 3 .. 6: LaunchConfig::tri_slab
// (0 = batched trilinear kernel, 1 / 3 / 4 = the LDS-staged kernel in one of its shapes).
// An entry settles on the fastest candidate after kTuneTries measurements of each (in an order shuffled per entry, so no
// candidate is always the one measured on cold clocks), is measured ONCE more kTuneRevalidateFrames frames later (the first
// ~25 frames after idle run ~15 % slow while the clocks ramp) and is evicted least-recently-used first.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <map>

#include "vr_frame.h"

namespace vr {

// the key of a launch: everything that shapes it; the pose enters through the view's axis alignment and the number of
// active tiles (buckets), so an orbiting camera re-uses what it has learnt.  rows: local image rows of the launch
// (launch_local_rows); prior: the heuristics' candidate bits
uint64_t launchTuneKey(const FrameParams &P, const LaunchConfig &L, int rows, unsigned tile_active, int prior);

// the blob of settled choices: one header, `count` records
struct ChoiceHeader { char magic[8]; uint32_t version, count; uint64_t build_id; char device[64]; };
struct ChoiceRecord { uint64_t key; int32_t ncand, settled_value, heur, cand[8]; };
static_assert(sizeof(ChoiceHeader) == 88 && sizeof(ChoiceRecord) == 56, "blob layout");

class LaunchTuner {
public:
    static constexpr int kTuneCand = 8, kTuneTries = 2, kTuneRevalidateFrames = 96, kTuneEntries = 512;
    static_assert(kTuneCand == 8, "ChoiceRecord::cand");
    struct TuneEntry {
        int ncand = 0, cand[kTuneCand] = {}, tries[kTuneCand] = {}, issued[kTuneCand] = {}, settled = -1, next = 0;   // issued: measurements launched (a burst of asynchronous frames launches kTuneTries per candidate, not one per frame until the results arrive)
        int heur = 0;                        // the heuristic's choice (a candidate value): it wins ties
        float best_ms[kTuneCand] = {};
        int frames_settled = 0;              // launches since it settled
        bool revalidated = false;
        uint64_t last_use = 0;               // launch counter at its last use (eviction order)
        uint64_t gen = 0;                    // generation: results of measurements launched for an earlier life of this key (evicted and re-created, or before a re-validation) are dropped
    };
    // what choose() decided for one launch
    struct Pick {
        bool decided = false;                // false: a configuration only passing through -- the launch stays as the heuristics set it
        int cand = 0;                        // the candidate VALUE (bit set) to launch, not its index in the entry's shuffled order
        bool measure = false;                // time this launch and report it: issued() once its events are recorded, record() with the result
        bool trial = false;                  // the configuration is still being explored (bit 8 of vr_get_launch_choice)
        uint64_t key = 0, gen = 0;           // what issued() / record() take back
    };

    // cand[0 .. n): the candidates of this launch, the heuristic's choice first (2 <= n <= kTuneCand); in_flight of `slots`
    // measurements are under way and have not reported.  Counts the launch: clock, run length of the key, eviction order
    Pick choose(uint64_t key, const int *cand, int n, int in_flight, int slots);
    void issued(uint64_t key, uint64_t gen, int cand_value);   // a measurement of `cand_value` was really launched (events recorded)
    void record(uint64_t key, uint64_t gen, int cand_value, float ms);

    // settled entries as a flat blob (vr_export_choices / vr_import_choices), ascending keys.  export: the bytes the blob needs,
    // written when capacity suffices.  import: entries accepted -- 0 for a blob of another build or device;
    // std::invalid_argument for one that is too short, not a choices blob, or truncated
    size_t exportChoices(void *buf, size_t capacity, uint64_t build_id, const char (&device)[64]) const;
    int importChoices(const void *buf, size_t bytes, uint64_t build_id, const char (&device)[64]);

    size_t entries() const { return tune_.size(); }
    const TuneEntry *find(uint64_t key) const { auto it = tune_.find(key); return it == tune_.end() ? nullptr : &it->second; }

private:
    std::map<uint64_t, TuneEntry> tune_;
    uint64_t tune_gen_counter_ = 0;
    uint64_t tune_clock_ = 0, tune_last_key_ = 0;   // launches seen; the previous launch's key and for how many launches in a row
    int tune_same_key_run_ = 0;
};

}  // namespace vr
