// TEST INFRASTRUCTURE ONLY -- runs the rank filter's pass schedule (volume-renderer_amd/csrc/rank_schedule.h) on the CPU; built by
// tests/test_rank_filter_cpu.py with g++ and the address and undefined-behaviour sanitizers.  One JSON line per run.
//   schedule_check schedule            every op 0 .. 5 with every zero / non-zero radius pattern (the non-zero radius: 1)
//   schedule_check refusals            rank_schedule's return value for arguments outside point 4 of the definition
//   schedule_check segment NA COLUMNS  rank_column_segment(NA, COLUMNS), any number of pairs
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "rank_schedule.h"

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    if (!std::strcmp(argv[1], "schedule")) {
        std::printf("[");
        for (int op = 0; op <= 5; op++)
            for (int m = 0; m < 8; m++) {
                const int r3[3] = {m & 1, m >> 1 & 1, m >> 2 & 1};
                vr::RankStep steps[vr::kRankMaxSteps + 1];
                const vr::RankStep guard = {-7, -7, -7, -7};
                for (int k = 0; k <= vr::kRankMaxSteps; k++) steps[k] = guard;
                const int n = vr::rank_schedule(op, r3, steps);
                if (n < 0 || n > vr::kRankMaxSteps || steps[vr::kRankMaxSteps].kernel != -7) return 3;
                std::printf("%s{\"op\": %d, \"r\": [%d, %d, %d], \"scratch\": %d, \"steps\": [", op || m ? ", " : "", op, r3[0], r3[1], r3[2],
                            vr::rank_scratch_buffers(steps, n));
                for (int k = 0; k < n; k++)
                    std::printf("%s[%d, %d, %d, %d]", k ? ", " : "", steps[k].kernel, steps[k].axis, steps[k].in, steps[k].out);
                std::printf("]}");
            }
        std::printf("]\n");
        return 0;
    }
    if (!std::strcmp(argv[1], "refusals")) {
        const int bad[][4] = {{-1, 1, 1, 1}, {6, 1, 1, 1}, {1, 9, 0, 0}, {2, 0, -1, 0}, {3, 0, 0, 9}, {4, 8, 8, 9}, {5, 2, 0, 0}, {5, 1, 1, 2}, {5, 0, -1, 0},
                                {0, 9, 0, 0}, {0, 0, 0, -1}};
        const int good[][4] = {{1, 8, 8, 8}, {4, 8, 0, 8}, {5, 1, 1, 1}, {0, 8, 8, 8}, {5, 0, 0, 0}, {3, 0, 0, 0}};
        vr::RankStep steps[vr::kRankMaxSteps];
        std::printf("{\"bad\": [");
        for (size_t t = 0; t < sizeof(bad) / sizeof(bad[0]); t++) std::printf("%s%d", t ? ", " : "", vr::rank_schedule(bad[t][0], &bad[t][1], steps));
        std::printf("], \"good\": [");
        for (size_t t = 0; t < sizeof(good) / sizeof(good[0]); t++) std::printf("%s%d", t ? ", " : "", vr::rank_schedule(good[t][0], &good[t][1], steps));
        std::printf("]}\n");
        return 0;
    }
    if (!std::strcmp(argv[1], "segment")) {
        std::printf("[");
        for (int a = 2; a + 1 < argc; a += 2)
            std::printf("%s%d", a > 2 ? ", " : "", vr::rank_column_segment(std::atoi(argv[a]), std::strtoull(argv[a + 1], nullptr, 10)));
        std::printf("]\n");
        return 0;
    }
    return 2;
}
