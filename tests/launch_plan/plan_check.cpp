// TEST INFRASTRUCTURE ONLY -- calls the launch rules (volume-renderer_amd/csrc/launch_plan.cpp) and the tile tables' rebuild
// rule (tile_schedule.cpp) with hand-made frames and prints what they decided as one JSON line; tests/test_launch_plan_cpu.py
// asserts on it.  Built by that test with g++ and the address / undefined-behaviour sanitizers; needs no GPU.
//   plan_check <scenario>     nearest | trilinear | candidates | bits | alpha | grid | rebuild
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "launch_plan.h"
#include "tile_schedule.h"

using namespace vr;

namespace {

struct Json {
    std::string s = "{";
    void key(const char *k) { if (s.size() > 1) s += ", "; s += "\""; s += k; s += "\": "; }
    void num(const char *k, long long v) { key(k); s += std::to_string(v); }
    void list(const char *k, const std::vector<long long> &v)
    {
        key(k); s += "[";
        for (size_t i = 0; i < v.size(); i++) { if (i) s += ", "; s += std::to_string(v[i]); }
        s += "]";
    }
    void print() { s += "}"; std::puts(s.c_str()); }
};

const uint32_t kTable[4] = {};                // something for the table / copy pointers to point at (never read)
const uint16_t kGrid[4] = {};

struct Frame { FrameParams P{}; LaunchConfig L{}; };

// an n^3 bricked volume in a unit box, grey ramp, certified divisions, window 0 .. 4095: eligible for the specialised kernel of
// its filter.  dir: the view matrix's third column -- with view_plane_dist 1 the central ray in voxel units is -n * dir, so the
// alignment is max |dir| / |dir|
Frame frame(int n, int bytes, int filter, float dx, float dy, float dz, float alpha)
{
    Frame f;
    FrameParams &P = f.P;
    P.cam[8] = dx; P.cam[9] = dy; P.cam[10] = dz; P.cam[20] = 1.0f;
    P.img_w = 320; P.img_h = 240; P.row_end = 240; P.stripe_rows = 1; P.stripe_count = 1;
    P.nx = P.ny = P.nz = n;
    P.bnx = P.bny = P.bnz = (n + 3) / 4;
    for (int a = 0; a < 3; a++) { P.ext[a] = 1.0f; P.pmin[a] = -0.5f; P.pmax[a] = 0.5f; }
    P.step = 1.0f / (float)n;
    P.alpha_scale = alpha;
    P.min_val = 0; P.max_val = 4095; P.fmin = 0.0f; P.fmax = 4095.0f; P.fden = 4095.0f;
    P.max_steps = 10000;
    f.L.bytes_per_voxel = bytes; f.L.filter = filter; f.L.layout = 1; f.L.divmode_tc = DIV_UNIT; f.L.divmode_win = DIV_CERT; f.L.use_lut = 1;
    f.L.tile_table = kTable;
    return f;
}

const float kAligned[3] = {0.0f, 0.0f, 1.0f}, kOblique[3] = {1.0f, 1.0f, 1.0f};   // alignment 1 and 0.577

long long nearestGuess(const float *d, float alpha, int variant, unsigned active, double longest)
{
    Frame f = frame(256, 2, 0, d[0], d[1], d[2], alpha);
    firstGuess(f.P, f.L, variant, active, longest);
    return choiceBits(f.L);
}

long long triGuess(int n, int bytes, float dx, float dy, float dz, bool small, int stripe_rows, int stripe_count, int variant, int preset)
{
    Frame f = frame(n, bytes, 1, dx, dy, dz, 0.02f);
    f.L.tri_slab = preset;
    if (small) f.L.tile_table_small = kTable;
    if (stripe_count > 1) { f.P.stripe_rows = stripe_rows; f.P.stripe_count = stripe_count; }
    firstGuess(f.P, f.L, variant, 100, 500.0);
    return f.L.tri_slab;
}

long long fallback(int shape, bool copy_y, bool copy_x, int tf_len, int variant)
{
    Frame f = frame(256, 2, 1, 0.6f, 0.8f, 1.0f, 0.02f);
    f.L.tri_slab = shape;
    f.P.tf_len = tf_len;
    if (copy_y) f.L.apron_y = kTable;
    if (copy_x) f.L.apron_x = kTable;
    halfLayerFallback(f.P, f.L, variant);
    return f.L.tri_slab;
}

std::vector<long long> candidates(const Frame &f, int prior)
{
    int c[kMaxCandidates + 1];
    c[kMaxCandidates] = -77;                                   // a guard behind the array
    const int n = launchCandidates(f.P, f.L, prior, c);
    std::vector<long long> v(c, c + n);
    if (c[kMaxCandidates] != -77) v.push_back(-77);
    return v;
}

// TRILINEAR with the apron copy and the optional things given
Frame triFrame(int bytes, const float *d, bool small, bool tall, bool copy_y, bool copy_x, int tf_len)
{
    Frame f = frame(256, bytes, 1, d[0], d[1], d[2], 0.02f);
    f.L.apron = kTable;
    f.P.tf_len = tf_len;
    if (small) f.L.tile_table_small = kTable;
    if (tall) f.L.tile_table_tall = kTable;
    if (copy_y) f.L.apron_y = kTable;
    if (copy_x) f.L.apron_x = kTable;
    return f;
}

void thresholds(Json &j, const char *name, float alpha, int min_val, int max_val, const float *lut)
{
    Frame f = frame(64, 2, 0, 0, 0, 1, alpha);
    f.P.min_val = min_val; f.P.max_val = max_val; f.P.fmin = (float)min_val; f.P.fmax = (float)max_val; f.P.fden = (float)(max_val - min_val);
    std::vector<long long> v;
    for (int whole = 0; whole < 2; whole++) {
        int t = -12345;
        const bool ok = zeroAlphaThreshold(f.P, min_val, max_val, lut, whole != 0, t);
        v.push_back(ok ? 1 : 0); v.push_back(ok ? t : 0);
    }
    j.list(name, v);                                                    // [ok, thresh] per value, then for the whole run
}

void grid(Json &j, const char *name, int nx, int ny, int nz)
{
    uint32_t c[3]; size_t total = 0;
    const bool ok = skipGridCells(nx, ny, nz, c, total);
    j.list(name, {ok ? 1 : 0, (long long)c[0], (long long)c[1], (long long)c[2], (long long)total});
}

long long withinCells(int nx, int ny, int nz, float e0, float e1, float e2, float step, int view_top)
{
    Frame f = frame(64, 2, 0, 0, 0, 1, 0.02f);
    f.P.nx = nx; f.P.ny = ny; f.P.nz = nz; f.P.ext[0] = e0; f.P.ext[1] = e1; f.P.ext[2] = e2; f.P.step = step; f.P.view_top = view_top;
    return nearestBatchWithinCells(f.P) ? 1 : 0;
}

}  // namespace

int main(int argc, char **argv)
{
    const std::string sc = argc > 1 ? argv[1] : "";
    Json j;
    if (sc == "nearest") {
        const struct { const float *d; double longest; unsigned active; } rows[] = {
            {kAligned, 1045.0, 255}, {kAligned, 1045.0, 256}, {kOblique, 1045.0, 1023}, {kOblique, 1045.0, 1024},
            {kAligned, 262.0, 67},   {kAligned, 262.0, 68},   {kAligned, 50.0, 38},     {kAligned, 50.0, 39}};
        std::vector<long long> lo, hi;
        for (const auto &r : rows) { lo.push_back(nearestGuess(r.d, 0.02f, 0, r.active, r.longest)); hi.push_back(nearestGuess(r.d, 0.5f, 0, r.active, r.longest)); }
        j.list("alpha_002", lo); j.list("alpha_05", hi);
        j.list("variant2", {nearestGuess(kAligned, 0.02f, 2, 0, 1045.0), nearestGuess(kAligned, 0.5f, 2, 255, 1045.0)});
        j.list("variant3", {nearestGuess(kAligned, 0.02f, 3, 256, 1045.0), nearestGuess(kOblique, 0.5f, 3, 100000, 1045.0)});
        j.list("variant5", {nearestGuess(kAligned, 0.02f, 5, 0, 1045.0), nearestGuess(kAligned, 1.0f, 5, 0, 1045.0), nearestGuess(kAligned, 1.0f, 5, 100000, 1045.0)});
        j.list("variant1", {nearestGuess(kAligned, 0.02f, 1, 255, 1045.0), nearestGuess(kAligned, 1.0f, 1, 256, 1045.0)});
    } else if (sc == "trilinear") {
        j.list("small", {triGuess(640, 2, 1, 1, 1, true, 0, 1, 0, 0), triGuess(641, 1, 1, 1, 1, true, 0, 1, 0, 0), triGuess(640, 1, 1, 1, 1, false, 0, 1, 0, 0),
                         triGuess(641, 1, 0, 0, 1, true, 0, 1, 0, 0)});
        j.list("u16_whole_layers", {triGuess(1024, 2, 0.17f, 0, 1, true, 0, 1, 0, 0), triGuess(1024, 2, 0.18f, 0, 1, true, 0, 1, 0, 0)});
        j.list("u16_ratios", {triGuess(1024, 2, 0.6f, 0.8f, 1, true, 0, 1, 0, 0), triGuess(1024, 2, 0.5f, 0.8f, 1, true, 0, 1, 0, 0),
                              triGuess(1024, 2, 0.6f, 0.69f, 1, true, 0, 1, 0, 0)});
        j.list("u16_stripes", {triGuess(1024, 2, 0.6f, 0.8f, 1, true, 16, 2, 0, 0), triGuess(1024, 2, 0.6f, 0.8f, 1, true, 32, 2, 0, 0)});
        j.list("variants", {triGuess(256, 2, 0.6f, 0.8f, 1, true, 0, 1, 8, 3), triGuess(256, 2, 0.6f, 0.8f, 1, true, 0, 1, 2, 0), triGuess(1024, 2, 0, 0, 1, true, 0, 1, 11, 6)});
        j.list("fallback", {fallback(3, false, false, 0, 0), fallback(4, true, false, 0, 0), fallback(3, false, true, 256, 0), fallback(4, false, false, 256, 0),
                            fallback(3, true, true, 0, 0), fallback(4, true, true, 256, 0), fallback(3, false, false, 0, 8), fallback(1, false, false, 0, 0),
                            fallback(6, false, false, 0, 0)});
    } else if (sc == "candidates") {
        Frame n = frame(256, 2, 0, 0, 0, 1, 0.02f);
        j.list("nearest_prior3", candidates(n, 3));
        Frame n1 = frame(256, 2, 0, 0, 0, 1, 1.0f);
        j.list("nearest_prior5_alpha1", candidates(n1, 5));
        Frame big = n; big.L.big_offsets = 1;
        j.list("big_offsets_prior3", candidates(big, 3));
        Frame skip = n; skip.P.skip_empty = 1; skip.L.skip_grid = kGrid;
        j.list("skipping_prior3", candidates(skip, 3));
        Frame grid_idle = n; grid_idle.L.skip_grid = kGrid;              // (a grid without skipping: the relay stays)
        j.list("grid_without_skipping_prior3", candidates(grid_idle, 3));
        Frame closed = n; closed.P.accum = 1;                            // closed-form accumulation: the generic kernel only
        j.list("generic_only", candidates(closed, 0));
        Frame no_apron = triFrame(2, kAligned, true, true, true, true, 0); no_apron.L.apron = nullptr;
        j.list("tri_no_apron", candidates(no_apron, 8));
        j.list("tri_base", candidates(triFrame(2, kAligned, false, false, false, false, 0), 8));
        j.list("tri_tf", candidates(triFrame(2, kAligned, false, false, false, false, 256), 8));
        j.list("tri_small", candidates(triFrame(2, kAligned, true, false, false, false, 256), 8));
        j.list("tri_copies", candidates(triFrame(2, kOblique, false, false, true, true, 256), 8));
        j.list("tri_copies_tall", candidates(triFrame(2, kOblique, false, true, true, true, 256), 8));
        j.list("tri_one_copy_tall", candidates(triFrame(2, kOblique, false, true, true, false, 256), 8));
        j.list("tri_u8_oblique_tall", candidates(triFrame(1, kOblique, false, true, false, false, 256), 8));
        j.list("tri_u8_aligned_tall", candidates(triFrame(1, kAligned, false, true, false, false, 256), 8));
        j.list("tri_u8_oblique_no_tall", candidates(triFrame(1, kOblique, false, false, false, false, 256), 8));
        j.list("tri_everything_prior16", candidates(triFrame(2, kOblique, true, true, true, true, 0), 16));
        j.list("tri_prior_first", candidates(triFrame(2, kOblique, true, true, true, true, 0), 32));
    } else if (sc == "bits") {
        std::vector<long long> bad;
        for (int filter = 0; filter < 2; filter++)
            for (int k = 0; k < (filter ? 7 : 8); k++) {
                const int c = filter ? k << 3 : k;
                Frame f = frame(64, 2, filter, 0, 0, 1, 0.02f);
                f.L.sparse_shard = f.L.pipelined = f.L.short_batches = 1; f.L.tri_slab = 9;   // (everything overwritten)
                applyChoice(f.L, c);
                const bool fields = f.L.sparse_shard == (c & 1) && f.L.pipelined == ((c >> 1) & 1) && f.L.short_batches == ((c >> 2) & 1) && f.L.tri_slab == (c >> 3);
                if (choiceBits(f.L) != c || !fields) bad.push_back(c);
            }
        j.list("not_inverse", bad);
        Frame t = frame(64, 2, 1, 0, 0, 1, 0.02f);
        t.L.sparse_shard = 1; t.L.pipelined = 1; t.L.tri_slab = 4;
        Frame n = t; n.L.filter = 0;
        j.list("trilinear_then_nearest", {choiceBits(t.L), choiceBits(n.L)});
    } else if (sc == "alpha") {
        std::vector<float> ten(1024, 0.0f), first(1024, 0.0f), narrow(1024, 0.0f);
        for (int e = 0; e < 256; e++) { ten[4 * e + 3] = e >= 10 ? 1.0f : 0.0f; first[4 * e + 3] = 1.0f; }
        narrow[4 * 64 + 3] = 1.0f;
        thresholds(j, "alpha_zero", 0.0f, 0, 255, first.data());
        thresholds(j, "grey_ramp", 0.5f, 37, 500, nullptr);
        thresholds(j, "ten_transparent", 0.5f, 0, 255, ten.data());
        thresholds(j, "entry0_visible", 0.5f, 0, 255, first.data());
        thresholds(j, "window_0_2", 0.5f, 0, 2, narrow.data());
    } else if (sc == "grid") {
        grid(j, "small", 100, 64, 9);
        grid(j, "x_last", 8 * ((1 << 24) - 1), 1, 1);
        grid(j, "x_first", 8 * ((1 << 24) - 1) + 1, 1, 1);
        grid(j, "yz_last", 8, 8 * 4096, 8 * 4095);
        grid(j, "yz_first", 8, 8 * 4096, 8 * 4095 + 1);
        grid(j, "total_last", 8 * 129, 8 * 4096, 8 * 4064);
        grid(j, "total_first", 8 * 129, 8 * 4096, 8 * 4064 + 1);
        const float s_in = 1.84375f / 128.0f, s_out = 1.859375f / 128.0f;   // exact in fp32
        j.list("batch_reach", {withinCells(128, 128, 128, 1, 1, 1, s_in, 0), withinCells(128, 128, 128, 1, 1, 1, s_out, 0),
                               withinCells(8, 8, 128, 1, 1, 2, s_out, 0), withinCells(8, 8, 128, 1, 1, 2, s_out, 1)});
    } else if (sc == "rebuild") {
        TileTablesBuilt b;
        b.table = true; b.shape_key = 7; b.skip_sig = 0;
        float cam[21] = {};
        auto stale = [&](const TileTablesBuilt &bb, uint64_t key, int64_t sig, bool tall, bool small) { return (long long)tileTablesStale(bb, key, cam, sig, tall, small); };
        std::vector<long long> drift;
        drift.push_back(stale(b, 7, 0, false, false));
        cam[13] = 0.05f; drift.push_back(stale(b, 7, 0, false, false));
        cam[13] = 0.0500001f; drift.push_back(stale(b, 7, 0, false, false));
        cam[13] = -0.0500001f; drift.push_back(stale(b, 7, 0, false, false));
        cam[13] = 0.0f; cam[0] = NAN; drift.push_back(stale(b, 7, 0, false, false));
        cam[0] = 0.0f; cam[20] = NAN; drift.push_back(stale(b, 7, 0, false, false));
        cam[20] = 0.0f;
        j.list("camera", drift);
        TileTablesBuilt none = b; none.table = false;
        j.list("key_and_table", {stale(b, 8, 0, false, false), stale(none, 7, 0, false, false)});
        TileTablesBuilt tall = b; tall.tall = true;
        TileTablesBuilt small = b; small.small = true;
        j.list("tall", {stale(b, 7, 0, true, false), stale(b, 7, 0, false, false), stale(tall, 7, 0, true, false), stale(small, 7, 0, true, false)});
        j.list("small", {stale(b, 7, 0, false, true), stale(small, 7, 0, false, true), stale(tall, 7, 0, false, true)});
        j.list("signature", {skipOrderSignature(0, 4095), skipOrderSignature(127, 4095), skipOrderSignature(128, 4095), skipOrderSignature(4095, 4095),
                             skipOrderSignature(-5, 4095), skipOrderSignature(65535, 65535), skipOrderSignature(3, -1)});
        TileTablesBuilt skipping = b; skipping.skip_sig = 1;
        TileTablesBuilt dropped = b; dropped.skip_sig = -1;
        j.list("signature_changes", {stale(skipping, 7, 1, false, false), stale(skipping, 7, 2, false, false), stale(skipping, 7, 0, false, false),
                                     stale(b, 7, 1, false, false), stale(dropped, 7, 1, false, false), stale(dropped, 7, 0, false, false)});
    } else {
        std::fprintf(stderr, "plan_check: unknown scenario '%s'\n", sc.c_str());
        return 2;
    }
    j.print();
    return 0;
}
