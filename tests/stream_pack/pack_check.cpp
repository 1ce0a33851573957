// pack_check.cpp -- a stand-alone check of csrc/vr_stream_pack.h: the pack / unpack pair the stream's record and replay kernels
// run, the choice of the stream's format and the size model.  Built for the host with -fsanitize=address,undefined and run
// directly by tests/test_ray_stream_pack_cpu.py; prints one line per failed check, exits non-zero if there was one.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "vr_stream_pack.h"

static int failures = 0;
#define CHECK(cond, ...)                                                          \
    do {                                                                          \
        if (!(cond)) { failures++; std::printf("FAIL %s:%d: %s -- ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    } while (0)

static uint32_t rng_state = 0x2545f491u;
static uint32_t rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

static void roundtrip(const uint32_t s[8], const char *what)
{
    uint32_t d[3];
    vr::stream_pack12(s, d);
    for (int u = 0; u < 8; u++) {
        const uint32_t got = vr::stream_unpack12(d[0], d[1], d[2], u);
        CHECK(got == s[u], "%s: position %d: packed %03x, unpacked %03x", what, u, s[u], got);
    }
    // the documented layout: one little-endian 96-bit number, sample u at bits [12 u, 12 u + 12)
    unsigned char bytes[12];
    std::memcpy(bytes, d, 12);             // (the kernels run on a little-endian device; so does this check)
    for (int u = 0; u < 8; u++) {
        uint32_t v = 0;
        for (int b = 0; b < 12; b++) {
            const int bit = 12 * u + b;
            v |= (uint32_t)((bytes[bit >> 3] >> (bit & 7)) & 1) << b;
        }
        CHECK(v == s[u], "%s: position %d: bits [%d, %d) hold %03x, not %03x", what, u, 12 * u, 12 * u + 12, v, s[u]);
    }
}

int main()
{
    static const uint32_t values[] = {0u, 1u, 0x555u, 0xaaau, 0xfffu};
    // every value at every position, its neighbours all ones and all zeros: a field that leaks into the next one shows
    for (int pos = 0; pos < 8; pos++)
        for (uint32_t v : values)
            for (uint32_t fill : {0u, 0xfffu}) {
                uint32_t s[8];
                for (int u = 0; u < 8; u++) s[u] = fill;
                s[pos] = v;
                roundtrip(s, fill ? "neighbours all ones" : "neighbours all zeros");
            }
    // the same value everywhere, alternating patterns
    for (uint32_t v : values) {
        uint32_t s[8];
        for (int u = 0; u < 8; u++) s[u] = v;
        roundtrip(s, "constant group");
        for (int u = 0; u < 8; u++) s[u] = (u & 1) ? v ^ 0xfffu : v;
        roundtrip(s, "alternating group");
    }
    for (int k = 0; k < 100000; k++) {
        uint32_t s[8];
        for (int u = 0; u < 8; u++) s[u] = rng() & 0xfffu;
        roundtrip(s, "random group");
    }

    // the format: span 4095 against 4096, u8 volumes, the three modes, one byte on either side of the threshold
    using vr::kStreamPack12; using vr::kStreamRaw; using vr::streamFormatFor;
    const uint64_t T = vr::kStreamPackMinRawBytes;
    CHECK(T == (256ull << 20), "threshold %llu", (unsigned long long)T);
    for (uint64_t bytes : {0ull, 1ull, (unsigned long long)T - 1, (unsigned long long)T, (unsigned long long)T + 1, 1ull << 40}) {
        for (int span : {0, 1, 4095}) {
            CHECK(streamFormatFor(0, 2, span, bytes) == kStreamRaw, "mode 0, span %d, %llu bytes", span, (unsigned long long)bytes);
            CHECK(streamFormatFor(2, 2, span, bytes) == kStreamPack12, "mode 2, span %d, %llu bytes", span, (unsigned long long)bytes);
            CHECK(streamFormatFor(1, 2, span, bytes) == (bytes > T ? kStreamPack12 : kStreamRaw), "mode 1, span %d, %llu bytes", span, (unsigned long long)bytes);
        }
        for (int mode = 0; mode <= 2; mode++) {
            CHECK(streamFormatFor(mode, 2, 4096, bytes) == kStreamRaw, "span 4096, mode %d", mode);
            CHECK(streamFormatFor(mode, 2, 65535, bytes) == kStreamRaw, "span 65535, mode %d", mode);
            CHECK(streamFormatFor(mode, 2, -1, bytes) == kStreamRaw, "an empty range, mode %d", mode);
            CHECK(streamFormatFor(mode, 1, 255, bytes) == kStreamRaw, "u8 volume, mode %d", mode);
            CHECK(streamFormatFor(mode, 1, 0, bytes) == kStreamRaw, "constant u8 volume, mode %d", mode);
        }
    }
    CHECK(vr::streamGroupOf(kStreamRaw) == 4u && vr::streamGroupOf(kStreamPack12) == 8u, "group sizes");

    // the size model: 12 bits per element of whole groups of 8 x 64 lanes; a multiple of 768 bytes
    for (uint64_t groups : {0ull, 1ull, 2ull, 29ull, 1000003ull, (1ull << 33) / 512ull + 7ull}) {
        const uint64_t elements = groups * 512ull;
        CHECK(vr::streamSampleBytes(kStreamPack12, 2, elements) == groups * 768ull, "%llu packed groups", (unsigned long long)groups);
        CHECK(vr::streamSampleBytes(kStreamRaw, 2, elements) == elements * 2ull, "%llu elements of 16 bits", (unsigned long long)elements);
        CHECK(vr::streamSampleBytes(kStreamRaw, 1, elements) == elements, "%llu elements of 8 bits", (unsigned long long)elements);
    }

    // the shifted window: inside the bound every constant is an exact float and the identity holds for every voxel; beyond it
    // the host must say so
    CHECK(vr::streamBaseFoldsIntoWindow(0, 4095, 0), "the headline's window");
    CHECK(vr::streamBaseFoldsIntoWindow(-100000, 100000, 65535), "a wide window, the largest base");
    CHECK(!vr::streamBaseFoldsIntoWindow(0, 1 << 24, 1000), "a window limit of 2^24");
    CHECK(!vr::streamBaseFoldsIntoWindow(-(1 << 24), 4095, 1000), "a window limit of -2^24");
    CHECK(!vr::streamBaseFoldsIntoWindow(0, 4095, -1), "a negative base");
    const int windows[][2] = {{0, 4095}, {1000, 5095}, {1500, 4000}, {-500, 700}, {0, 999}, {6000, 9000}, {-(1 << 23), 1 << 23}};
    for (const auto &w : windows)
        for (int base : {0, 1, 1000, 61440}) {
            if (!vr::streamBaseFoldsIntoWindow(w[0], w[1], base)) { CHECK(false, "window [%d, %d] base %d is inside the bound", w[0], w[1], base); continue; }
            const float fmin = (float)w[0], fmax = (float)w[1];
            const volatile float sfmin = fmin - (float)base, sfmax = fmax - (float)base;
            for (int t = 0; t <= 4095; t++) {
                const float v = (float)(t + base);
                const volatile float a = (v < fmin ? fmin : v > fmax ? fmax : v) - fmin;
                const float p = (float)t;
                const volatile float b = (p < sfmin ? sfmin : p > sfmax ? sfmax : p) - sfmin;
                const float fa = a, fb = b;
                if (std::memcmp(&fa, &fb, 4) != 0) { CHECK(false, "window [%d, %d] base %d sample %d: %a vs %a", w[0], w[1], base, t, (double)fa, (double)fb); break; }
            }
        }

    if (failures == 0) std::printf("pack_check: ok\n");
    return failures == 0 ? 0 : 1;
}
