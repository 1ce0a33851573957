// launch_tuner.cpp -- see launch_tuner.h.
//
// ---- the measured work model.  Which kernel is fastest for a launch depends on how many tiles have work, how long
// their rays are, how early they end and how oblique the view is (tools/config_sweep.py: the relay kernel wins a
// 1024^3 shard with 171 active tiles by 25 %, loses a 256^3 frame with 560 by 45 %).  Round 2 chose by tile-count
// thresholds fitted on one configuration; here the launch is MEASURED: all candidates render identical bits, so the
// first frames of a configuration try them in turn (the heuristic's choice first), a few times each, and the fastest
// is kept.  Keyed by everything that shapes the launch; the pose enters through the view's axis alignment and the
// number of active tiles (buckets), so an orbiting camera re-uses what it has learnt.
#include "launch_tuner.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <utility>
#include <vector>

#include "tile_schedule.h"

namespace vr {

uint64_t launchTuneKey(const FrameParams &P, const LaunchConfig &L, int rows, unsigned tile_active, int prior)
{
    uint64_t key = tileScheduleKey(P, rows, false);
    auto mix = [&](uint64_t v) { key ^= v + 0x9E3779B97F4A7C15ull + (key << 6) + (key >> 2); };
    mix((uint64_t)(viewAxisAlignment(P) * 25.0));
    if (L.filter == 1) {
        // the staged trilinear kernel's time follows how many tiles' brick layers fit its ring, i.e. HOW the view is oblique
        // (orbit poses of one alignment bucket: 1.2 ... 2.5 ms on a 1024^3 u8 volume): both direction ratios, in eighths
        double r1, r2;
        viewAxisRatios(P, r1, r2);
        mix((uint64_t)(r1 * 8.0) << 8 | (uint64_t)(r2 * 8.0));
    }
    mix((uint64_t)(std::log2((double)std::max(tile_active, 1u)) * 3.0));
    // opacity and window enter in coarse buckets (how early rays end, how wide the classification table is): a slider dragged
    // through hundreds of values stays in one or two entries instead of opening a new one -- and a new exploration -- per frame
    const double a = (double)P.alpha_scale;
    mix((uint64_t)(a >= 0.5 ? 1000 : (a > 0.0 ? (int)std::floor(std::log2(a) * 0.5) + 500 : 0)));
    mix((uint64_t)std::floor(std::log2((double)std::max(P.max_val - P.min_val, 1))) << 8 | (uint64_t)(L.use_lut != 0) << 1 | (uint64_t)(L.lut_noclamp != 0));
    mix((uint64_t)P.nx << 40 | (uint64_t)P.ny << 20 | (uint64_t)P.nz);
    mix((uint64_t)L.filter | (uint64_t)L.mip << 1 | (uint64_t)(P.tf_len > 1) << 2 | (uint64_t)(P.skip_empty != 0) << 3 | (uint64_t)L.layout << 4 |
        (uint64_t)L.bytes_per_voxel << 5 | (uint64_t)(L.packed12 != nullptr) << 8 | (uint64_t)(L.apron != nullptr) << 9 | (uint64_t)P.fb_format << 10 |
        (uint64_t)P.view_top << 11 | (uint64_t)P.view_bottom << 12 | (uint64_t)(L.apron_y != nullptr) << 13 | (uint64_t)prior << 16);
    return key;
}

void LaunchTuner::issued(uint64_t key, uint64_t gen, int cand_value)
{
    auto it = tune_.find(key);
    if (it == tune_.end() || it->second.gen != gen) return;
    for (int c = 0; c < it->second.ncand; c++) if (it->second.cand[c] == cand_value) { it->second.issued[c]++; return; }
}

// `cand_value` is the candidate's bit set, `gen` the entry's generation when the measurement was launched: an entry that was
// evicted and re-created for the same key has another shuffled order (an index would credit the wrong candidate), and a
// result launched before a re-validation must not count towards it (round-4 advisor)
void LaunchTuner::record(uint64_t key, uint64_t gen, int cand_value, float ms)
{
    auto it = tune_.find(key);
    if (it == tune_.end() || it->second.gen != gen) return;
    int cand = -1;
    for (int c = 0; c < it->second.ncand; c++) if (it->second.cand[c] == cand_value) cand = c;
    if (cand < 0) return;
    TuneEntry &e = it->second;
    e.best_ms[cand] = e.tries[cand] == 0 ? ms : std::min(e.best_ms[cand], ms);
    e.tries[cand]++;
    bool all = true;
    for (int c = 0; c < e.ncand; c++) all = all && e.tries[c] >= kTuneTries;
    if (all) {
        // the heuristic's choice wins ties: a rival has to be 2 % faster, more than two event timings of one kernel differ by
        int heur = 0;
        for (int c = 0; c < e.ncand; c++) if (e.cand[c] == e.heur) heur = c;
        int best = heur;
        for (int c = 0; c < e.ncand; c++)
            if (c != heur && e.best_ms[c] < e.best_ms[best] * (best == heur ? 0.98f : 1.0f)) best = c;
        e.settled = best;
        e.frames_settled = 0;
    }
}

LaunchTuner::Pick LaunchTuner::choose(uint64_t key, const int *cand, int n, int in_flight, int slots)
{
    Pick p;
    tune_clock_++;
    tune_same_key_run_ = key == tune_last_key_ ? tune_same_key_run_ + 1 : 0;
    tune_last_key_ = key;
    auto it = tune_.find(key);
    if (it == tune_.end()) {
        // a configuration that is only passing through (an orbiting camera crossing a pose bucket, a slider crossing an opacity
        // bucket) gets the heuristic's choice; exploring starts when the same key has come three times in a row
        if (tune_same_key_run_ < 2) return p;
        if (tune_.size() >= (size_t)kTuneEntries) {                      // evict the least recently used eighth
            std::vector<std::pair<uint64_t, uint64_t>> age;
            age.reserve(tune_.size());
            for (auto &kv : tune_) age.emplace_back(kv.second.last_use, kv.first);
            std::nth_element(age.begin(), age.begin() + kTuneEntries / 8, age.end());
            for (int k = 0; k < kTuneEntries / 8; k++) tune_.erase(age[(size_t)k].second);
        }
        it = tune_.emplace(key, TuneEntry{}).first;
        TuneEntry &e = it->second;
        e.ncand = n;
        e.gen = ++tune_gen_counter_;
        for (int k = 0; k < n; k++) e.cand[k] = cand[k];
        e.heur = cand[0];
        // shuffled measuring order (Fisher-Yates on a counter-seeded LCG)
        uint64_t r = key ^ (tune_clock_ * 0x9E3779B97F4A7C15ull);
        for (int k = n - 1; k > 0; k--) {
            r = r * 6364136223846793005ull + 1442695040888963407ull;
            std::swap(e.cand[k], e.cand[(int)((r >> 33) % (uint64_t)(k + 1))]);
        }
    }
    TuneEntry &e = it->second;
    e.last_use = tune_clock_;
    int use;
    if (e.settled >= 0) {
        use = e.settled;
        // one re-measurement at sustained clocks: whatever settled during the clock ramp is checked again, once
        if (!e.revalidated && ++e.frames_settled >= kTuneRevalidateFrames) {
            e.revalidated = true;
            for (int c = 0; c < e.ncand; c++) { e.tries[c] = 0; e.issued[c] = 0; e.best_ms[c] = 0.0f; }
            e.settled = -1;
            e.next = 0;
            e.gen = ++tune_gen_counter_;                                 // results still in flight belong to the old generation
        }
    } else {
        // the next candidate that still needs a measurement launched; when every measurement is in flight (a burst of
        // asynchronous frames) or every event pair is taken: the best so far, the heuristic's choice before any result
        int pick = -1;
        if (in_flight < slots)
            for (int k = 0; k < e.ncand && pick < 0; k++) {
                const int c = (e.next + k) % e.ncand;
                if (e.issued[c] < kTuneTries) pick = c;
            }
        if (pick >= 0) {
            use = pick;
            e.next = (pick + 1) % e.ncand;
            // issued[] is counted where the event pair is really recorded (the caller's issued()): a launch that cannot
            // measure (the instrumented sample count, every slot taken) leaves the candidate to be picked again
            p.measure = true;
        } else {
            int best = -1;
            for (int c = 0; c < e.ncand; c++)
                if (e.tries[c] > 0 && (best < 0 || e.best_ms[c] < e.best_ms[best])) best = c;
            if (best < 0)
                for (int c = 0; c < e.ncand; c++) if (e.cand[c] == e.heur) best = c;
            use = best < 0 ? 0 : best;
            // a measurement whose events were lost (a failed launch) would leave the entry waiting for ever: with nothing in
            // flight, whatever has not reported is launched again
            if (in_flight == 0)
                for (int c = 0; c < e.ncand; c++) if (e.tries[c] < kTuneTries) e.issued[c] = e.tries[c];
        }
    }
    p.decided = true;
    p.cand = e.cand[use];
    p.trial = e.settled < 0;                                             // (also the launch that starts the re-validation: it runs the old settled candidate)
    p.key = key;
    p.gen = e.gen;
    return p;
}

// ---- settled choices as a blob.  The reference dispatches ONE shader per frame and never tries anything
// (src/RendererCore.cpp:138-163); with an imported table neither does this library for the configurations the table knows.
size_t LaunchTuner::exportChoices(void *buf, size_t capacity, uint64_t build_id, const char (&device)[64]) const
{
    uint32_t n = 0;
    for (const auto &kv : tune_) if (kv.second.settled >= 0) n++;
    const size_t need = sizeof(ChoiceHeader) + (size_t)n * sizeof(ChoiceRecord);
    if (!buf || capacity < need) return need;
    ChoiceHeader h;
    std::memset(&h, 0, sizeof(h));
    std::memcpy(h.magic, "VRCHOICE", 8);
    h.version = 1; h.count = n; h.build_id = build_id;
    std::memcpy(h.device, device, sizeof(h.device));
    std::memcpy(buf, &h, sizeof(h));
    char *q = static_cast<char *>(buf) + sizeof(h);
    for (const auto &kv : tune_) {
        const TuneEntry &e = kv.second;
        if (e.settled < 0) continue;
        ChoiceRecord r;
        std::memset(&r, 0, sizeof(r));
        r.key = kv.first; r.ncand = e.ncand; r.settled_value = e.cand[e.settled]; r.heur = e.heur;
        for (int c = 0; c < e.ncand; c++) r.cand[c] = e.cand[c];
        std::memcpy(q, &r, sizeof(r));
        q += sizeof(r);
    }
    return need;
}

int LaunchTuner::importChoices(const void *buf, size_t bytes, uint64_t build_id, const char (&device)[64])
{
    if (!buf || bytes < sizeof(ChoiceHeader)) throw std::invalid_argument("importChoices: blob too short");
    ChoiceHeader h;
    std::memcpy(&h, buf, sizeof(h));
    if (std::memcmp(h.magic, "VRCHOICE", 8) != 0 || h.version != 1) throw std::invalid_argument("importChoices: not a choices blob of this library");
    if (bytes < sizeof(h) + (size_t)h.count * sizeof(ChoiceRecord)) throw std::invalid_argument("importChoices: truncated blob");
    if (h.build_id != build_id || std::memcmp(h.device, device, sizeof(device)) != 0) return 0;   // measured elsewhere: not trusted
    const char *q = static_cast<const char *>(buf) + sizeof(h);
    int accepted = 0;
    for (uint32_t i = 0; i < h.count && tune_.size() < (size_t)kTuneEntries; i++, q += sizeof(ChoiceRecord)) {
        ChoiceRecord r;
        std::memcpy(&r, q, sizeof(r));
        if (r.ncand < 2 || r.ncand > kTuneCand) continue;
        int settled = -1;
        for (int c = 0; c < r.ncand; c++) if (r.cand[c] == r.settled_value) settled = c;
        if (settled < 0) continue;
        TuneEntry e;
        e.ncand = r.ncand; e.heur = r.heur; e.settled = settled;
        for (int c = 0; c < r.ncand; c++) { e.cand[c] = r.cand[c]; e.tries[c] = e.issued[c] = kTuneTries; }
        e.revalidated = true;                                            // it was measured at sustained clocks where it came from
        e.last_use = tune_clock_;
        e.gen = ++tune_gen_counter_;
        tune_[r.key] = e;
        accepted++;
    }
    return accepted;
}

}  // namespace vr
