// TEST INFRASTRUCTURE ONLY -- instantiates the helpers of volume-renderer_amd/csrc/mode_dispatch.h with a functor that records
// the template arguments it is called with, sweeps every runtime combination and prints what it saw as one JSON line;
// tests/test_mode_dispatch_cpu.py asserts on it.  Built by that test with g++ and the address / undefined-behaviour
// sanitizers, linked with launch_plan.cpp (launch_local_rows); needs no GPU and no HIP header.
//   dispatch_check <scenario>     sweep | tiles | divmodes
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "mode_dispatch.h"

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

#define V(c) decltype(c)::value   // the constant an axis handed over

// what an instance is: its template arguments, as the kernels take them
template <int LAYOUT, int FILTER, bool FLAG, int MODE, bool BIG>
long long instance() { return LAYOUT * 10000 + FILTER * 1000 + (FLAG ? 100 : 0) + MODE * 10 + (BIG ? 1 : 0); }

// layout x filter x flag x big x reslice's three modes: every runtime combination, each through the helpers the launchers use
void sweep(Json &j)
{
    std::vector<long long> asked, got;
    long long calls = 0;
    for (int layout = 0; layout < 2; layout++)
        for (int filter = 0; filter < 2; filter++)
            for (int flag = 0; flag < 2; flag++)
                for (int big = 0; big < 2; big++)
                    for (int mode = 0; mode < 3; mode++) {
                        LaunchConfig L{};
                        L.layout = layout; L.filter = filter; L.big_offsets = big;
                        asked.push_back(layout * 10000 + filter * 1000 + flag * 100 + mode * 10 + big);
                        // the flag as the extra axis (iso, shade), inside it the mode as the extra axis (reslice)
                        got.push_back(dispatch_mode(L, BoolAxis{flag != 0}, [&](auto LAY, auto FIL, auto FLAG, auto BIG) {
                            return dispatch_mode(L, IntAxis<3>{mode}, [&](auto LAY2, auto FIL2, auto MODE, auto BIG2) {
                                calls++;
                                if (V(LAY) != V(LAY2) || V(FIL) != V(FIL2) || V(BIG) != V(BIG2)) return -1ll;
                                return instance<V(LAY), V(FIL), V(FLAG), V(MODE), V(BIG)>();
                            });
                        }));
                    }
    j.num("calls", calls);
    j.list("asked", asked);
    j.list("got", got);
    // the switches are "0 or not": any other layout / filter is 1, any other big_offsets true; a mode past 1 is the last instance
    LaunchConfig L{};
    L.layout = 2; L.filter = -1; L.big_offsets = 7;
    j.num("not_zero", dispatch_mode(L, IntAxis<3>{5}, [](auto LAY, auto FIL, auto MODE, auto BIG) { return instance<V(LAY), V(FIL), false, V(MODE), V(BIG)>(); }));
    // the axes arrive in the order they are given
    j.num("order", dispatch([](auto a, auto b, auto c) { return (long long)(V(a) * 100 + V(b) * 10 + (V(c) ? 1 : 0)); }, IntAxis<3>{2}, IntAxis<2>{0}, BoolAxis{true}));
    j.num("no_axis", dispatch([] { return 7ll; }));
}

// 16x16-pixel tiles: ceil(width / 16) x ceil(rows / 16), rows from launch_local_rows (a row range, then cyclic stripes)
void tiles(Json &j)
{
    const int sizes[5] = {0, 1, 15, 16, 17};
    std::vector<long long> one, x, y;
    for (int n : sizes) one.push_back(tiles16(n));
    for (int w : sizes)
        for (int rows : sizes) {
            FrameParams P{};
            P.img_w = w; P.img_h = 64; P.row_begin = 5; P.row_end = 5 + rows; P.stripe_rows = 1; P.stripe_count = 1;
            const Tiles16 t = launch_tiles16(P);
            x.push_back(t.x); y.push_back(t.y);
        }
    j.list("tiles16", one);
    j.list("x", x);
    j.list("y", y);
    // stripes of 8 rows dealt to 2 ranks over 40 image rows: rank 0 has stripes 0, 2, 4 (24 local rows: 2 tile rows), rank 1
    // stripes 1, 3 (16 local rows: 1)
    std::vector<long long> striped;
    for (int rank = 0; rank < 2; rank++) {
        FrameParams P{};
        P.img_w = 17; P.img_h = 40; P.stripe_rows = 8; P.stripe_count = 2; P.stripe_index = rank;
        const Tiles16 t = launch_tiles16(P);
        striped.push_back(t.x); striped.push_back(t.y);
    }
    j.list("striped", striped);
}

// texture coordinates: certified unless exact; the window: exact unless certified
void divmodes(Json &j)
{
    std::vector<long long> tc, win;
    for (int d : {(int)DIV_UNIT, (int)DIV_CERT, (int)DIV_EXACT}) {
        LaunchConfig L{};
        L.divmode_tc = d; L.divmode_win = d;
        tc.push_back(texcoord_divmode(L)); win.push_back(window_divmode(L));
    }
    j.list("texcoord", tc);
    j.list("window", win);
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    Json j;
    if (!std::strcmp(argv[1], "sweep")) sweep(j);
    else if (!std::strcmp(argv[1], "tiles")) tiles(j);
    else if (!std::strcmp(argv[1], "divmodes")) divmodes(j);
    else return 2;
    j.print();
    return 0;
}
