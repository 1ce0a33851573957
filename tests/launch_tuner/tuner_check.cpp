// TEST INFRASTRUCTURE ONLY -- drives vr::LaunchTuner (volume-renderer_amd/csrc/launch_tuner.cpp) through one scenario with
// synthetic millisecond values and prints what happened as one JSON line; tests/test_launch_tuner_cpu.py asserts on it.
// Built by that test with g++ and the address / undefined-behaviour sanitizers; needs no GPU.
//   tuner_check <scenario>     pass | settle | burst | lost | stale | reval | evict | blob | keys
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "launch_tuner.h"

using vr::LaunchTuner;
using Pick = vr::LaunchTuner::Pick;

namespace {

constexpr int kSlots = 12;                   // RendererCore's ring of event pairs
const int kCands[3] = {4, 0, 1};             // the heuristic's choice first
const char kDevice[64] = "cc9.5 cu256 test device";
constexpr uint64_t kBuild = 0x0123456789abcdefull;

// ---- a JSON object, built field by field
struct Json {
    std::string s = "{";
    void key(const char *k) { if (s.size() > 1) s += ", "; s += "\""; s += k; s += "\": "; }
    void num(const char *k, long long v) { key(k); s += std::to_string(v); }
    void flag(const char *k, bool v) { key(k); s += v ? "true" : "false"; }
    template <class T> void list(const char *k, const std::vector<T> &v)
    {
        key(k); s += "[";
        for (size_t i = 0; i < v.size(); i++) { if (i) s += ", "; s += std::to_string((long long)v[i]); }
        s += "]";
    }
    void print() { s += "}"; std::puts(s.c_str()); }
};

// the same key until the tuner decides: returns the deciding (third) pick
Pick decide(LaunchTuner &t, uint64_t key, const int *cand = kCands, int n = 3)
{
    Pick p;
    for (int i = 0; i < 3 && !p.decided; i++) p = t.choose(key, cand, n, 0, kSlots);
    return p;
}

// the blocking path: every measurement is issued and recorded at once, ms[candidate value] = its successive timings.
// `first` is a pick already taken; returns the number of measurements per candidate value
std::map<int, int> measureAll(LaunchTuner &t, uint64_t key, Pick first, const std::map<int, std::vector<float>> &ms, const int *cand = kCands, int n = 3)
{
    std::map<int, int> count;
    Pick p = first;
    for (int guard = 0; guard < 100 && p.measure; guard++) {
        const std::vector<float> &v = ms.at(p.cand);
        const float x = v[(size_t)count[p.cand] % v.size()];
        count[p.cand]++;
        t.issued(p.key, p.gen, p.cand);
        t.record(p.key, p.gen, p.cand, x);
        if (t.find(key)->settled >= 0) break;
        p = t.choose(key, cand, n, 0, kSlots);
    }
    return count;
}

int settledValue(const LaunchTuner &t, uint64_t key)
{
    const LaunchTuner::TuneEntry *e = t.find(key);
    return (e && e->settled >= 0) ? e->cand[e->settled] : -1;
}

int settleOn(LaunchTuner &t, uint64_t key, const std::map<int, std::vector<float>> &ms)
{
    measureAll(t, key, decide(t, key), ms);
    return settledValue(t, key);
}

// ---- scenarios
void pass()
{
    Json j;
    LaunchTuner a;
    std::vector<int> decided;
    for (int i = 0; i < 12; i++) decided.push_back(a.choose(i % 2 ? 200 : 100, kCands, 3, 0, kSlots).decided);
    j.list("alternating_decided", decided);
    j.num("alternating_entries", (long long)a.entries());
    // A A B A A: never three in a row; the next A is the third
    LaunchTuner b;
    std::vector<int> d2, m2;
    for (uint64_t k : {100, 100, 200, 100, 100, 100}) {
        const Pick p = b.choose(k, kCands, 3, 0, kSlots);
        d2.push_back(p.decided); m2.push_back(p.measure);
        if (!p.decided) { d2.back() = (p.cand == 0 && !p.measure && !p.trial) ? 0 : -1; }   // an undecided pick carries nothing
    }
    j.list("run_decided", d2);
    j.list("run_measure", m2);
    j.num("run_entries", (long long)b.entries());
    j.flag("run_entry_is_A", b.find(100) != nullptr && b.find(200) == nullptr);
    LaunchTuner c;
    const Pick p = decide(c, 100);
    j.flag("third_decided", p.decided); j.flag("third_measure", p.measure); j.flag("third_trial", p.trial);
    j.num("third_key", (long long)p.key);
    j.print();
}

void settle()
{
    Json j;
    { LaunchTuner t; j.num("rival_0985", settleOn(t, 1, {{4, {1.0f}}, {0, {0.985f}}, {1, {1.2f}}})); }
    { LaunchTuner t; j.num("rival_097", settleOn(t, 1, {{4, {1.0f}}, {0, {0.97f}}, {1, {1.2f}}})); }
    { LaunchTuner t; j.num("rivals_09_08", settleOn(t, 1, {{4, {1.0f}}, {0, {0.9f}}, {1, {0.8f}}})); }
    { LaunchTuner t; j.num("rivals_08_09", settleOn(t, 1, {{4, {1.0f}}, {0, {0.8f}}, {1, {0.9f}}})); }
    { LaunchTuner t; j.num("heuristic_fastest", settleOn(t, 1, {{4, {0.5f}}, {0, {0.8f}}, {1, {0.9f}}})); }
    // a candidate's time is the minimum of its measurements: 0 wins by its second, 1 loses in spite of neither
    { LaunchTuner t; j.num("minimum_counts", settleOn(t, 1, {{4, {1.0f, 2.0f}}, {0, {3.0f, 0.9f}}, {1, {0.95f, 0.95f}}})); }
    LaunchTuner t;
    const Pick first = decide(t, 7);
    const std::map<int, int> count = measureAll(t, 7, first, {{4, {1.0f}}, {0, {0.5f}}, {1, {1.2f}}});
    std::vector<int> per;
    for (int c : kCands) per.push_back(count.count(c) ? count.at(c) : 0);
    j.list("measurements_per_candidate", per);
    const Pick after = t.choose(7, kCands, 3, 0, kSlots);
    j.flag("after_decided", after.decided); j.num("after_cand", after.cand);
    j.flag("after_measure", after.measure); j.flag("after_trial", after.trial);
    j.print();
}

void burst()
{
    Json j;
    LaunchTuner t;
    int in_flight = 0;
    std::vector<int> measure, cand, trial;
    Pick p = decide(t, 5);
    for (int i = 0; i < 11; i++) {
        if (i) p = t.choose(5, kCands, 3, in_flight, kSlots);
        measure.push_back(p.measure); cand.push_back(p.cand); trial.push_back(p.trial);
        if (p.measure) { t.issued(p.key, p.gen, p.cand); in_flight++; }
    }
    j.list("measure", measure); j.list("cand", cand); j.list("trial", trial);
    std::vector<int> issued, tries;
    for (int c = 0; c < 3; c++) { issued.push_back(t.find(5)->issued[c]); tries.push_back(t.find(5)->tries[c]); }
    j.list("issued", issued); j.list("tries", tries);
    // every event pair taken: nothing can be measured, nothing counts as issued
    LaunchTuner f;
    std::vector<int> fmeasure, fcand;
    p = f.choose(6, kCands, 3, kSlots, kSlots); p = f.choose(6, kCands, 3, kSlots, kSlots);
    for (int i = 0; i < 8; i++) {
        p = f.choose(6, kCands, 3, kSlots, kSlots);
        fmeasure.push_back(p.measure); fcand.push_back(p.decided ? p.cand : -1);
    }
    j.list("full_measure", fmeasure); j.list("full_cand", fcand);
    std::vector<int> fissued;
    for (int c = 0; c < 3; c++) fissued.push_back(f.find(6)->issued[c]);
    j.list("full_issued", fissued);
    j.print();
}

void lost()
{
    Json j;
    LaunchTuner t;
    Pick p = decide(t, 5);
    int launched = 0;
    while (p.measure && launched < 20) { t.issued(p.key, p.gen, p.cand); launched++; p = t.choose(5, kCands, 3, launched, kSlots); }
    j.num("launched", launched);
    j.flag("waiting_measure", p.measure);
    // the results never arrive, and nothing is in flight any more
    const Pick rearm = t.choose(5, kCands, 3, 0, kSlots);
    j.flag("rearm_measure", rearm.measure); j.num("rearm_cand", rearm.cand);
    std::vector<int> issued;
    for (int c = 0; c < 3; c++) issued.push_back(t.find(5)->issued[c]);
    j.list("issued_after_rearm", issued);
    const Pick again = t.choose(5, kCands, 3, 0, kSlots);
    j.flag("again_measure", again.measure);
    const std::map<int, int> count = measureAll(t, 5, again, {{4, {1.0f}}, {0, {0.5f}}, {1, {1.2f}}});
    int total = 0;
    for (auto &kv : count) total += kv.second;
    j.num("measured_after", total);
    j.num("settled", settledValue(t, 5));
    j.print();
}

void fillTable(LaunchTuner &t, uint64_t base, int n)
{
    for (int i = 0; i < n; i++) decide(t, base + (uint64_t)i);
}

void stale()
{
    Json j;
    // (a) a result launched before the re-validation
    LaunchTuner t;
    const Pick first = decide(t, 9);
    measureAll(t, 9, first, {{4, {1.0f}}, {0, {0.5f}}, {1, {1.2f}}});
    Pick p;
    for (int i = 0; i < LaunchTuner::kTuneRevalidateFrames; i++) p = t.choose(9, kCands, 3, 0, kSlots);
    j.flag("revalidating", p.trial && t.find(9)->settled < 0);
    j.flag("generation_changed", t.find(9)->gen != first.gen);
    for (int rep = 0; rep < 2; rep++)
        for (int c : kCands) { t.issued(9, first.gen, c); t.record(9, first.gen, c, 0.001f); }
    int sum = 0;
    for (int c = 0; c < 3; c++) sum += t.find(9)->tries[c] + t.find(9)->issued[c];
    j.num("counts_after_stale_results", sum);
    j.num("settled_after_stale_results", t.find(9)->settled);
    // (b) an evicted and re-created key
    LaunchTuner u;
    const Pick old = decide(u, 9);
    u.issued(old.key, old.gen, old.cand);
    fillTable(u, 1000, LaunchTuner::kTuneEntries);      // the 512th of these evicts key 9, the oldest
    j.flag("evicted", u.find(9) == nullptr);
    const Pick fresh = decide(u, 9);
    j.flag("recreated", u.find(9) != nullptr && fresh.measure);
    j.flag("recreated_generation_differs", fresh.gen != old.gen);
    for (int rep = 0; rep < 2; rep++)
        for (int c : kCands) { u.issued(9, old.gen, c); u.record(9, old.gen, c, 0.001f); }
    sum = 0;
    for (int c = 0; c < 3; c++) sum += u.find(9)->tries[c] + u.find(9)->issued[c];
    j.num("recreated_counts_after_stale_results", sum);
    j.num("recreated_settled", u.find(9)->settled);
    j.print();
}

std::vector<unsigned char> exported(const LaunchTuner &t, uint64_t build = kBuild, const char (&device)[64] = kDevice)
{
    std::vector<unsigned char> b(t.exportChoices(nullptr, 0, build, device));
    t.exportChoices(b.data(), b.size(), build, device);
    return b;
}

void reval()
{
    Json j;
    LaunchTuner t;
    j.num("settled_first", settleOn(t, 3, {{4, {1.0f}}, {0, {0.5f}}, {1, {1.2f}}}));
    int fired_at = -1;
    Pick p;
    for (int i = 1; i <= 200 && fired_at < 0; i++) {
        p = t.choose(3, kCands, 3, 0, kSlots);
        if (p.trial) fired_at = i;
    }
    j.num("fired_at", fired_at);
    j.num("firing_cand", p.cand); j.flag("firing_measure", p.measure); j.flag("firing_decided", p.decided);
    // fresh measurements, with another winner
    p = t.choose(3, kCands, 3, 0, kSlots);
    j.flag("next_measure", p.measure); j.flag("next_trial", p.trial);
    const std::map<int, int> count = measureAll(t, 3, p, {{4, {1.0f}}, {0, {1.5f}}, {1, {0.6f}}});
    int total = 0;
    for (auto &kv : count) total += kv.second;
    j.num("remeasured", total);
    j.num("settled_second", settledValue(t, 3));
    int trials = 0, other = 0;
    for (int i = 0; i < 400; i++) {
        p = t.choose(3, kCands, 3, 0, kSlots);
        trials += p.trial; other += p.cand != 1 || p.measure;
    }
    j.num("trials_afterwards", trials); j.num("other_picks_afterwards", other);
    // an imported entry: decided from the first call, never re-validated
    LaunchTuner v;
    const std::vector<unsigned char> blob = exported(t);
    j.num("imported", v.importChoices(blob.data(), blob.size(), kBuild, kDevice));
    trials = other = 0;
    for (int i = 0; i < 400; i++) {
        p = v.choose(3, kCands, 3, 0, kSlots);
        trials += p.trial; other += !p.decided || p.cand != 1 || p.measure;
    }
    j.num("imported_trials", trials); j.num("imported_other_picks", other);
    j.print();
}

void evict()
{
    Json j;
    LaunchTuner t;
    const int n = LaunchTuner::kTuneEntries;
    std::vector<int> want((size_t)n);
    for (int i = 0; i < n; i++) {
        const int winner = kCands[i % 3];
        std::map<int, std::vector<float>> ms;
        for (int c : kCands) ms[c] = {c == winner ? 0.5f : 1.0f};
        want[(size_t)i] = settleOn(t, 1000 + (uint64_t)i, ms);
    }
    j.num("entries_before", (long long)t.entries());
    for (int i = 0; i < 32; i++) t.choose(1000 + (uint64_t)i, kCands, 3, 0, kSlots);   // the 32 oldest are used again
    const Pick p = decide(t, 5000);
    j.flag("new_decided", p.decided && t.find(5000) != nullptr);
    j.num("entries_after", (long long)t.entries());
    std::vector<int> missing;
    int changed = 0;
    for (int i = 0; i < n; i++) {
        if (!t.find(1000 + (uint64_t)i)) missing.push_back(i);
        else changed += settledValue(t, 1000 + (uint64_t)i) != want[(size_t)i] || want[(size_t)i] != kCands[i % 3];
    }
    j.list("missing", missing);
    j.num("survivors_changed", changed);
    j.print();
}

std::vector<unsigned char> craft(const std::vector<vr::ChoiceRecord> &recs)
{
    vr::ChoiceHeader h;
    std::memset(&h, 0, sizeof(h));
    std::memcpy(h.magic, "VRCHOICE", 8);
    h.version = 1; h.count = (uint32_t)recs.size(); h.build_id = kBuild;
    std::memcpy(h.device, kDevice, sizeof(h.device));
    std::vector<unsigned char> b(sizeof(h) + recs.size() * sizeof(vr::ChoiceRecord));
    std::memcpy(b.data(), &h, sizeof(h));
    if (!recs.empty()) std::memcpy(b.data() + sizeof(h), recs.data(), recs.size() * sizeof(vr::ChoiceRecord));
    return b;
}

vr::ChoiceRecord rec(uint64_t key, int ncand, int settled_value)
{
    vr::ChoiceRecord r;
    std::memset(&r, 0, sizeof(r));
    r.key = key; r.ncand = ncand; r.settled_value = settled_value; r.heur = 4;
    const int c[8] = {4, 0, 1, 2, 8, 24, 40, 48};
    for (int k = 0; k < 8; k++) r.cand[k] = c[k];
    return r;
}

int tryImport(LaunchTuner &t, const std::vector<unsigned char> &b, size_t bytes, uint64_t build = kBuild, const char (&device)[64] = kDevice)
{
    try { return t.importChoices(b.data(), bytes, build, device); }
    catch (const std::invalid_argument &) { return -1; }               // -1: refused
}

void blob()
{
    Json j;
    j.num("sizeof_header", (long long)sizeof(vr::ChoiceHeader));
    j.num("sizeof_record", (long long)sizeof(vr::ChoiceRecord));
    LaunchTuner t;
    const uint64_t keys[5] = {0xfffffffffffffff0ull, 40, 7, 0x123456789ull, 300};
    for (int i = 0; i < 5; i++) {
        std::map<int, std::vector<float>> ms;
        for (int c : kCands) ms[c] = {c == kCands[i % 3] ? 0.5f : 1.0f};
        settleOn(t, keys[i], ms);
    }
    decide(t, 55);                                                       // still exploring: not exported
    const size_t need = t.exportChoices(nullptr, 0, kBuild, kDevice);
    j.num("need", (long long)need);
    std::vector<unsigned char> small(need - 1, 0xAA);
    j.num("need_small_buffer", (long long)t.exportChoices(small.data(), small.size(), kBuild, kDevice));
    bool untouched = true;
    for (unsigned char c : small) untouched = untouched && c == 0xAA;
    j.flag("small_buffer_untouched", untouched);
    const std::vector<unsigned char> b = exported(t);
    j.flag("magic", std::memcmp(b.data(), "VRCHOICE", 8) == 0);
    std::vector<int> ascending;
    for (size_t i = 0; i + 1 < 5; i++) {
        uint64_t k0, k1;
        std::memcpy(&k0, b.data() + 88 + 56 * i, 8); std::memcpy(&k1, b.data() + 88 + 56 * (i + 1), 8);
        ascending.push_back(k0 < k1);
    }
    j.list("ascending", ascending);
    LaunchTuner u;
    j.num("accepted", tryImport(u, b, b.size()));
    j.num("entries", (long long)u.entries());
    j.flag("round_trip_identical", exported(u) == b);
    const LaunchTuner::TuneEntry *e = u.find(40);
    j.flag("imported_state", e && e->revalidated && e->tries[0] == 2 && e->tries[2] == 2 && e->issued[1] == 2 && e->settled >= 0);
    j.num("accepted_again", tryImport(u, b, b.size()));             // overwrites, still counted
    j.num("entries_again", (long long)u.entries());
    LaunchTuner w;
    std::vector<unsigned char> other = b;
    other[16] ^= 0x5a;
    j.num("other_build", tryImport(w, other, other.size()));
    char device2[64] = "cc9.4 cu304 another device";
    j.num("other_device", tryImport(w, b, b.size(), kBuild, device2));
    j.num("entries_after_foreign", (long long)w.entries());
    other = b; other[7] = 'X';
    j.num("bad_magic", tryImport(w, other, other.size()));
    other[16] ^= 0x5a;
    j.num("bad_magic_other_build", tryImport(w, other, other.size()));   // the magic is checked first
    other = b; other[8] = 2;
    j.num("bad_version", tryImport(w, other, other.size()));
    j.num("short_87", tryImport(w, b, 87));
    j.num("cut_in_records", tryImport(w, b, b.size() - 1));
    j.num("cut_in_records_other_build", tryImport(w, b, 100, kBuild + 1));   // truncation is checked before the build id
    j.num("entries_after_refused", (long long)w.entries());
    // records that are skipped, the others still taken
    LaunchTuner x;
    const std::vector<unsigned char> mixed = craft({rec(1, 1, 4), rec(2, 3, 0), rec(3, 9, 4), rec(4, 3, 2), rec(5, 8, 48), rec(6, 0, 4), rec(7, 2, 1)});
    j.num("mixed_accepted", tryImport(x, mixed, mixed.size()));
    std::vector<int> present;
    for (uint64_t k = 1; k <= 7; k++) present.push_back(x.find(k) != nullptr);
    j.list("mixed_present", present);
    j.num("mixed_settled_2", settledValue(x, 2)); j.num("mixed_settled_5", settledValue(x, 5));
    // the table takes 512 entries
    std::vector<vr::ChoiceRecord> many;
    for (int i = 0; i < 600; i++) many.push_back(rec(10000 + (uint64_t)i, 3, 1));
    LaunchTuner y;
    const std::vector<unsigned char> big = craft(many);
    j.num("many_accepted", tryImport(y, big, big.size()));
    j.num("many_entries", (long long)y.entries());
    j.print();
}

void keys()
{
    Json j;
    vr::FrameParams P;
    vr::LaunchConfig L;
    std::memset(&P, 0, sizeof(P));
    std::memset(&L, 0, sizeof(L));
    // the slider-drag configuration: a 512^3 u16 bricked volume, 1920 x 1080, the camera on the z axis
    P.cam[0] = 1.0f; P.cam[5] = 1.0f; P.cam[10] = 1.0f; P.cam[19] = 3.0f; P.cam[20] = 1.0f;
    P.img_w = 1920; P.img_h = 1080; P.row_begin = 0; P.row_end = 1080; P.col_lim = 1920; P.row_lim = 1080;
    P.stripe_rows = 0; P.stripe_index = 0; P.stripe_count = 1;
    P.nx = P.ny = P.nz = 512;
    for (int a = 0; a < 3; a++) { P.fdim[a] = 512.0f; P.half[a] = 0.5f; P.pmin[a] = -0.5f; P.pmax[a] = 0.5f; P.ext[a] = 1.0f; P.rext[a] = 1.0f; }
    P.step = 1.0f / 512.0f; P.max_steps = 10000;
    P.alpha_scale = 0.02f; P.min_val = 0; P.max_val = 4095;
    L.bytes_per_voxel = 2; L.filter = 0; L.layout = 1; L.use_lut = 1; L.lut_noclamp = 1;
    const int rows = 1080, prior = 2;
    const unsigned active = 2000;
    const uint64_t base = vr::launchTuneKey(P, L, rows, active, prior);
    auto with = [&](auto change) { vr::FrameParams p = P; vr::LaunchConfig l = L; change(p, l); return vr::launchTuneKey(p, l, rows, active, prior); };
    j.flag("deterministic", base == vr::launchTuneKey(P, L, rows, active, prior));
    j.flag("alpha_002_002239_same", base == with([](vr::FrameParams &p, vr::LaunchConfig &) { p.alpha_scale = 0.02239f; }));
    j.flag("alpha_002_006_same", base == with([](vr::FrameParams &p, vr::LaunchConfig &) { p.alpha_scale = 0.06f; }));   // one bucket: [1/64, 1/16)
    j.flag("alpha_002_01_differ", base != with([](vr::FrameParams &p, vr::LaunchConfig &) { p.alpha_scale = 0.1f; }));
    j.flag("alpha_05_1_same", with([](vr::FrameParams &p, vr::LaunchConfig &) { p.alpha_scale = 0.5f; }) == with([](vr::FrameParams &p, vr::LaunchConfig &) { p.alpha_scale = 1.0f; }));
    j.flag("alpha_05_differs_from_002", base != with([](vr::FrameParams &p, vr::LaunchConfig &) { p.alpha_scale = 0.5f; }));
    j.flag("width_4095_3856_same", base == with([](vr::FrameParams &p, vr::LaunchConfig &) { p.max_val = 3856; }));
    j.flag("width_4095_2047_differ", base != with([](vr::FrameParams &p, vr::LaunchConfig &) { p.max_val = 2047; }));
    j.flag("nx_differs", base != with([](vr::FrameParams &p, vr::LaunchConfig &) { p.nx = 511; }));
    j.flag("filter_differs", base != with([](vr::FrameParams &, vr::LaunchConfig &l) { l.filter = 1; }));
    j.flag("layout_differs", base != with([](vr::FrameParams &, vr::LaunchConfig &l) { l.layout = 0; }));
    j.flag("prior_differs", base != vr::launchTuneKey(P, L, rows, active, 3));
    j.flag("rows_differ", base != vr::launchTuneKey(P, L, 540, active, prior));
    j.flag("active_tiles_bucket_same", base == vr::launchTuneKey(P, L, rows, 2040, prior));   // floor(3 log2): 32 for both
    j.flag("active_tiles_differ", base != vr::launchTuneKey(P, L, rows, 500, prior));
    j.print();
}

}  // namespace

int main(int argc, char **argv)
{
    const std::string s = argc > 1 ? argv[1] : "";
    if (s == "pass") pass();
    else if (s == "settle") settle();
    else if (s == "burst") burst();
    else if (s == "lost") lost();
    else if (s == "stale") stale();
    else if (s == "reval") reval();
    else if (s == "evict") evict();
    else if (s == "blob") blob();
    else if (s == "keys") keys();
    else { std::fprintf(stderr, "tuner_check: unknown scenario '%s'\n", s.c_str()); return 2; }
    return 0;
}
