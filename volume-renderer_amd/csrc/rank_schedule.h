// rank_schedule.h -- which passes one vr_rank_filter_volume runs, along which axis, from which buffer to which (DESIGN.md
// section 1.9).  Plain C++, no HIP: volume_rank.cpp launches what this says, tests/rank_schedule/schedule_check.cpp checks it
// on the CPU under the sanitizers.
#pragma once

namespace vr {

constexpr int kRankOff = 0, kRankErode = 1, kRankDilate = 2, kRankOpen = 3, kRankClose = 4, kRankMedian = 5;   // VR_RANK_*
constexpr int kRankMaxRadius = 8;                        // ERODE, DILATE, OPEN, CLOSE; the column kernels' LDS ring is sized by it
constexpr int kRankMaxMedianRadius = 1;
constexpr int kRankMaxSteps = 6;                         // OPEN and CLOSE along three axes

enum RankKernel { RANK_MIN = 0, RANK_MAX = 1, RANK_MEDIAN = 2 };
enum RankBuffer { RANK_SRC = 0, RANK_DST = 1, RANK_TMP0 = 2, RANK_TMP1 = 3 };

struct RankStep {
    int kernel;                                          // RankKernel
    int axis;                                            // 0 x, 1 y, 2 z; -1: the median's one launch over the whole box
    int in, out;                                         // RankBuffer
};

// op in 0 .. 5 and every radius in 0 .. 8 (0 .. 1 for MEDIAN)
inline bool rank_arguments_ok(int op, const int r3[3])
{
    if (op < kRankOff || op > kRankMedian) return false;
    const int hi = op == kRankMedian ? kRankMaxMedianRadius : kRankMaxRadius;
    for (int a = 0; a < 3; a++)
        if (r3[a] < 0 || r3[a] > hi) return false;
    return true;
}

// the identity: OFF, or a box of one voxel
inline bool rank_is_identity(int op, const int r3[3]) { return op == kRankOff || (r3[0] == 0 && r3[1] == 0 && r3[2] == 0); }

// The steps of (op, r3) into steps[kRankMaxSteps]; returns their number, 0 for the identity, -1 for refused arguments.
// Minimum and maximum over a box are separable: one pass per axis with r > 0, in the order x, y, z; OPEN is that for the
// minimum and then for the maximum, CLOSE the other way round; MEDIAN is one launch.  The passes alternate between dst and one
// scratch volume such that the last one writes dst: no pass works in place, src is only ever read, and RANK_TMP1 is never used.
inline int rank_schedule(int op, const int r3[3], RankStep steps[kRankMaxSteps])
{
    if (!rank_arguments_ok(op, r3)) return -1;
    if (rank_is_identity(op, r3)) return 0;
    int n = 0;
    if (op == kRankMedian) {
        steps[n++] = RankStep{RANK_MEDIAN, -1, RANK_SRC, RANK_DST};
        return n;
    }
    const int first = (op == kRankErode || op == kRankOpen) ? RANK_MIN : RANK_MAX;
    const int stages = (op == kRankOpen || op == kRankClose) ? 2 : 1;
    for (int s = 0; s < stages; s++)
        for (int a = 0; a < 3; a++)
            if (r3[a] > 0) steps[n++] = RankStep{s == 0 ? first : (first == RANK_MIN ? RANK_MAX : RANK_MIN), a, 0, 0};
    for (int k = 0; k < n; k++) {
        steps[k].out = (n - 1 - k) % 2 == 0 ? RANK_DST : RANK_TMP0;
        steps[k].in = k == 0 ? RANK_SRC : steps[k - 1].out;
    }
    return n;
}

// Outputs along the axis per workgroup of a y or z pass over columns of `na` voxels, `columns` workgroups across them: one
// workgroup per column where the columns alone give 2048 workgroups (eight per CU); else the column is halved into segments,
// each a multiple of 16 outputs and not below 48 (a segment reads 2r halo rows again).  The Gaussian's rule, equally untuned.
inline int rank_column_segment(int na, unsigned long long columns)
{
    int seg = (na + 15) / 16 * 16;
    while (seg > 64 && columns * (unsigned long long)((na + seg - 1) / seg) < 2048) seg = (seg / 2 + 15) / 16 * 16;
    return seg;
}

// scratch volumes the schedule needs (0 or 1)
inline int rank_scratch_buffers(const RankStep *steps, int n)
{
    int most = 0;
    for (int k = 0; k < n; k++) {
        if (steps[k].in >= RANK_TMP0 && steps[k].in - RANK_TMP0 + 1 > most) most = steps[k].in - RANK_TMP0 + 1;
        if (steps[k].out >= RANK_TMP0 && steps[k].out - RANK_TMP0 + 1 > most) most = steps[k].out - RANK_TMP0 + 1;
    }
    return most;
}

}  // namespace vr
