// mode_dispatch.h -- the launch scaffold of the single-kernel modes (vr_iso.hip, vr_reslice.hip, vr_shade.hip): the runtime
// switches of a launch become template arguments once, in one place; with them the 16x16-pixel tile count and the two division
// modes those launchers pass on.  Host-only and HIP-free, so the mapping is tested without a device (tests/mode_dispatch).
#pragma once
#include <type_traits>

#include "launch_plan.h"   // launch_local_rows
#include "vr_frame.h"

namespace vr {

// an int switch with N instances: 0 .. N - 2 as they are, anything else the last (layout, filter: "not 0" is 1)
template <int N>
struct IntAxis {
    int v;
    template <int I = 0, class F>
    decltype(auto) visit(F &&f) const
    {
        if constexpr (I + 1 < N) {
            if (v == I) return f(std::integral_constant<int, I>{});
            return visit<I + 1>(f);
        } else {
            return f(std::integral_constant<int, I>{});
        }
    }
};
struct BoolAxis {
    bool v;
    template <class F>
    decltype(auto) visit(F &&f) const { return v ? f(std::true_type{}) : f(std::false_type{}); }
};

// f(c0, c1, ...) with one std::integral_constant per axis, in the axes' order
template <class F>
decltype(auto) dispatch(F &&f) { return f(); }
template <class F, class Axis, class... Rest>
decltype(auto) dispatch(F &&f, Axis a, Rest... rest)
{
    return a.visit([&](auto c) { return dispatch([&](auto... cs) { return f(c, cs...); }, rest...); });
}

// the axes every single-kernel mode has, around its own: f(LAYOUT, FILTER, extra, BIG)
template <class Axis, class F>
decltype(auto) dispatch_mode(const LaunchConfig &L, Axis extra, F &&f)
{
    return dispatch(f, IntAxis<2>{L.layout}, IntAxis<2>{L.filter}, extra, BoolAxis{L.big_offsets != 0});
}

// 16x16-pixel tiles over the image's width and the rows of this launch
struct Tiles16 { unsigned x, y; };
inline unsigned tiles16(int n) { return (unsigned)((n + 15) / 16); }
inline Tiles16 launch_tiles16(const FrameParams &P) { return Tiles16{tiles16(P.img_w), tiles16(launch_local_rows(P))}; }

// what the generic-shaped kernels take: texture coordinates certified unless exact, the window exact unless certified
inline int texcoord_divmode(const LaunchConfig &L) { return L.divmode_tc == DIV_EXACT ? DIV_EXACT : DIV_CERT; }
inline int window_divmode(const LaunchConfig &L) { return L.divmode_win == DIV_CERT ? DIV_CERT : DIV_EXACT; }

}  // namespace vr
