// key_check.cpp -- rayGeometryKey (launch_plan.cpp) field by field: prints one JSON line, {"changes": {field: 0 | 1, ...},
// "keeps": {field: 0 | 1, ...}, ...}; 1 = the key differs from the base launch's after that field alone was changed.
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "launch_plan.h"

using namespace vr;

static void base(FrameParams &P, LaunchConfig &L)
{
    std::memset(&P, 0, sizeof(P));
    std::memset(&L, 0, sizeof(L));
    for (int i = 0; i < 21; i++) P.cam[i] = 0.25f * (float)(i + 1);
    P.img_w = 96; P.img_h = 80; P.row_begin = 0; P.row_end = 80; P.col_lim = 96; P.row_lim = 80;
    P.stripe_rows = 1; P.stripe_index = 0; P.stripe_count = 1;
    P.nx = 40; P.ny = 52; P.nz = 36;
    for (int a = 0; a < 3; a++) { P.half[a] = 0.5f; P.pmin[a] = -0.5f; P.pmax[a] = 0.5f; P.ext[a] = 1.0f; P.rext[a] = 1.0f; }
    P.step = 0.001f; P.max_steps = 10000;
    P.alpha_scale = 0.004f; P.min_val = 0; P.max_val = 4095; P.fmin = 0.0f; P.fmax = 4095.0f; P.fden = 4095.0f; P.rden = 1.0f / 4095.0f;
    L.bytes_per_voxel = 2; L.layout = 1; L.divmode_tc = DIV_UNIT; L.divmode_win = DIV_CERT;
}

int main()
{
    struct Case { std::string name; std::function<void(FrameParams &, LaunchConfig &, uint64_t &)> change; };
    std::vector<Case> changes, keeps;
    auto C = [&](const char *n, std::function<void(FrameParams &, LaunchConfig &, uint64_t &)> f) { changes.push_back({n, f}); };
    auto K = [&](const char *n, std::function<void(FrameParams &, LaunchConfig &, uint64_t &)> f) { keeps.push_back({n, f}); };
    for (int i = 0; i < 21; i++) {
        const std::string n = "cam" + std::to_string(i);
        changes.push_back({n, [i](FrameParams &P, LaunchConfig &, uint64_t &) { uint32_t b; std::memcpy(&b, &P.cam[i], 4); b ^= 1u; std::memcpy(&P.cam[i], &b, 4); }});   // one ulp
    }
    C("img_w", [](FrameParams &P, LaunchConfig &, uint64_t &) { P.img_w++; });
    C("img_h", [](FrameParams &P, LaunchConfig &, uint64_t &) { P.img_h++; });
    C("row_begin", [](FrameParams &P, LaunchConfig &, uint64_t &) { P.row_begin++; });
    C("row_end", [](FrameParams &P, LaunchConfig &, uint64_t &) { P.row_end--; });
    C("col_lim", [](FrameParams &P, LaunchConfig &, uint64_t &) { P.col_lim--; });
    C("row_lim", [](FrameParams &P, LaunchConfig &, uint64_t &) { P.row_lim--; });
    C("stripe_rows", [](FrameParams &P, LaunchConfig &, uint64_t &) { P.stripe_rows = 16; });
    C("stripe_index", [](FrameParams &P, LaunchConfig &, uint64_t &) { P.stripe_index = 1; });
    C("stripe_count", [](FrameParams &P, LaunchConfig &, uint64_t &) { P.stripe_count = 3; });
    C("nx", [](FrameParams &P, LaunchConfig &, uint64_t &) { P.nx++; });
    C("ny", [](FrameParams &P, LaunchConfig &, uint64_t &) { P.ny++; });
    C("nz", [](FrameParams &P, LaunchConfig &, uint64_t &) { P.nz++; });
    for (int a = 0; a < 3; a++) {
        const std::string s = std::to_string(a);
        changes.push_back({"half" + s, [a](FrameParams &P, LaunchConfig &, uint64_t &) { P.half[a] = 0.25f; }});
        changes.push_back({"pmin" + s, [a](FrameParams &P, LaunchConfig &, uint64_t &) { P.pmin[a] = -0.25f; }});
        changes.push_back({"pmax" + s, [a](FrameParams &P, LaunchConfig &, uint64_t &) { P.pmax[a] = 0.25f; }});
        changes.push_back({"ext" + s, [a](FrameParams &P, LaunchConfig &, uint64_t &) { P.ext[a] = 0.5f; }});
        changes.push_back({"rext" + s, [a](FrameParams &P, LaunchConfig &, uint64_t &) { P.rext[a] = 2.0f; }});
    }
    C("step", [](FrameParams &P, LaunchConfig &, uint64_t &) { P.step = 0.002f; });
    C("max_steps", [](FrameParams &P, LaunchConfig &, uint64_t &) { P.max_steps = 9999; });
    C("view_top", [](FrameParams &P, LaunchConfig &, uint64_t &) { P.view_top = 1; });
    C("view_bottom", [](FrameParams &P, LaunchConfig &, uint64_t &) { P.view_bottom = 1; });
    C("divmode_tc", [](FrameParams &, LaunchConfig &L, uint64_t &) { L.divmode_tc = DIV_CERT; });
    C("layout", [](FrameParams &, LaunchConfig &L, uint64_t &) { L.layout = 0; });
    C("bytes_per_voxel", [](FrameParams &, LaunchConfig &L, uint64_t &) { L.bytes_per_voxel = 1; });
    C("generation", [](FrameParams &, LaunchConfig &, uint64_t &g) { g++; });
    C("generation_high_word", [](FrameParams &, LaunchConfig &, uint64_t &g) { g += 1ull << 32; });

    K("window", [](FrameParams &P, LaunchConfig &L, uint64_t &) { P.min_val = 100; P.max_val = 900; P.fmin = 100.0f; P.fmax = 900.0f; P.fden = 800.0f; P.rden = 1.0f / 800.0f; L.lut_noclamp = 1; L.use_lut = 1; });
    K("alpha", [](FrameParams &P, LaunchConfig &, uint64_t &) { P.alpha_scale = 1.0f; });
    K("tf_len", [](FrameParams &P, LaunchConfig &, uint64_t &) { P.tf_len = 256; P.tf_grey = 1; });
    K("accum", [](FrameParams &P, LaunchConfig &, uint64_t &) { P.accum = 1; });
    K("fb_compact", [](FrameParams &P, LaunchConfig &, uint64_t &) { P.fb_compact = 1; });
    K("fb_format", [](FrameParams &P, LaunchConfig &, uint64_t &) { P.fb_format = 1; });
    K("pk12_base", [](FrameParams &P, LaunchConfig &L, uint64_t &) { P.pk12_base = 1000; L.packed12 = &P; L.packed12_bytes = 64; });
    K("mip", [](FrameParams &, LaunchConfig &L, uint64_t &) { L.mip = 1; });
    K("variant_bits", [](FrameParams &, LaunchConfig &L, uint64_t &) { L.sparse_shard = 1; L.pipelined = 1; L.short_batches = 1; });

    FrameParams P0; LaunchConfig L0;
    base(P0, L0);
    const RayGeometryKey k0 = rayGeometryKey(P0, L0, 7);
    FrameParams P1; LaunchConfig L1;
    base(P1, L1);
    const int same = rayGeometryKey(P1, L1, 7) == k0 ? 1 : 0;        // two launches of one geometry: equal keys
    std::printf("{\"same\": %d, \"words\": %d", same, RayGeometryKey::kWords);
    for (int pass = 0; pass < 2; pass++) {
        std::printf(", \"%s\": {", pass == 0 ? "changes" : "keeps");
        const std::vector<Case> &v = pass == 0 ? changes : keeps;
        for (size_t i = 0; i < v.size(); i++) {
            FrameParams P; LaunchConfig L; uint64_t gen = 7;
            base(P, L);
            v[i].change(P, L, gen);
            std::printf("%s\"%s\": %d", i ? ", " : "", v[i].name.c_str(), rayGeometryKey(P, L, gen) != k0 ? 1 : 0);
        }
        std::printf("}");
    }
    // eligibility: the fast kernel's frames with a tile table and the skipping switch off
    L0.tile_table = reinterpret_cast<const uint32_t *>(&P0);
    const int ok = rayStreamEligible(P0, L0, 0) ? 1 : 0, skipping = rayStreamEligible(P0, L0, 1) ? 1 : 0;
    L0.filter = 1;
    const int trilinear = rayStreamEligible(P0, L0, 0) ? 1 : 0;
    L0.filter = 0; L0.tile_table = nullptr;
    const int no_table = rayStreamEligible(P0, L0, 0) ? 1 : 0;
    std::printf(", \"eligible\": [%d, %d, %d, %d]}\n", ok, skipping, trilinear, no_table);
    return 0;
}
