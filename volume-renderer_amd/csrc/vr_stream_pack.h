// vr_stream_pack.h -- the 12-bit packed format of the ray-ordered sample stream (vr_stream.hip): the pack /
// unpack pair the record and replay kernels run, the host's choice of the format and the size model.  Plain C++ without a HIP
// header, so that a CPU program (tests/stream_pack/pack_check.cpp) tests exactly what the kernels run.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VR_PACK_HD __host__ __device__
#else
#define VR_PACK_HD
#endif

namespace vr {

// A packed sample is voxel - base in 12 bits (base: the volume's exact minimum; lossless when exact_max - exact_min <= 4095).
// A group is 8 samples = 96 bits = three dwords per lane, read as ONE little-endian 96-bit number: sample u is bits
// [12 u, 12 u + 12).  d0 = s0 | s1 << 12 | s2 << 24, d1 = s2 >> 8 | s3 << 4 | s4 << 16 | s5 << 28, d2 = s5 >> 4 | s6 << 8 | s7 << 20.
// Unpacking is six bit-field extracts and, for the two samples that straddle a dword (s2, s5), a funnel shift and a mask each.
constexpr unsigned kStreamGroup12 = 8;
constexpr int kStreamSpan12 = 4095;             // the largest exact_max - exact_min the format holds

enum StreamFormat { kStreamRaw = 0, kStreamPack12 = 1 };

// s[u] < 4096
VR_PACK_HD inline void stream_pack12(const uint32_t s[8], uint32_t d[3])
{
    d[0] = s[0] | (s[1] << 12) | (s[2] << 24);
    d[1] = (s[2] >> 8) | (s[3] << 4) | (s[4] << 16) | (s[5] << 28);
    d[2] = (s[5] >> 4) | (s[6] << 8) | (s[7] << 20);
}

// sample u (0 .. 7; a constant where the kernels call it) of the group (d0, d1, d2)
VR_PACK_HD inline uint32_t stream_unpack12(uint32_t d0, uint32_t d1, uint32_t d2, int u)
{
    switch (u) {
    case 0: return d0 & 0xfffu;
    case 1: return (d0 >> 12) & 0xfffu;
    case 2: return (uint32_t)((((uint64_t)d1 << 32) | d0) >> 24) & 0xfffu;
    case 3: return (d1 >> 4) & 0xfffu;
    case 4: return (d1 >> 16) & 0xfffu;
    case 5: return (uint32_t)((((uint64_t)d2 << 32) | d1) >> 28) & 0xfffu;
    case 6: return (d2 >> 8) & 0xfffu;
    default: return d2 >> 20;
    }
}

// The automatic rule (vr_set_ray_stream_pack 1) packs a stream whose 16-bit form is larger than the device's last-level cache
// (256 MiB of Infinity Cache on MI355X): beyond it a replayed frame reads the stream from HBM and its time is the byte count;
// below it nothing has been measured to say so.  The largest 16-bit stream an existing test builds under the default mode --
// and asserts to the byte -- has 11 892 736 sample bytes (600 x 456 pixels of the 64^3 noise ball; tests/ray_stream_cases.py's
// model, computed by tests/test_ray_stream_pack_cpu.py), a twentieth of the threshold; 600 x 456 pixels x 200 samples (more
// than any ray through the unit box has) x 2 bytes = 109 MB bounds them all.
constexpr uint64_t kStreamPackMinRawBytes = 256ull << 20;

// The format of a stream: mode 0 never packs, 1 is the automatic rule, 2 packs whenever the format is lossless for the volume.
// span = exact_max - exact_min of the volume; raw_sample_bytes: the samples of the stream in its 16-bit form (groups of 4).
inline StreamFormat streamFormatFor(int mode, int bytes_per_voxel, int64_t span, uint64_t raw_sample_bytes)
{
    if (mode == 0 || bytes_per_voxel != 2 || span < 0 || span > kStreamSpan12) return kStreamRaw;
    if (mode == 2) return kStreamPack12;
    return raw_sample_bytes > kStreamPackMinRawBytes ? kStreamPack12 : kStreamRaw;
}

inline unsigned streamGroupOf(StreamFormat f) { return f == kStreamPack12 ? kStreamGroup12 : 4u; }

// bytes of `elements` samples (padding included: whole groups for all 64 lanes of every block), without the 16 bytes of slack
inline uint64_t streamSampleBytes(StreamFormat f, int bytes_per_voxel, uint64_t elements)
{
    return f == kStreamPack12 ? elements / 2u * 3u : elements * (uint64_t)bytes_per_voxel;
}

// The arithmetic classification of a packed sample t = voxel - base shifts the window instead of adding the base back:
//   clamp(float(voxel), fmin, fmax) - fmin  ==  clamp(float(t), fmin - base, fmax - base) - (fmin - base)   bit for bit
// when min_val, max_val, base and voxel are integers whose sums and differences here stay below 2^24 in magnitude: then
// float(min_val), fmin - base, fmax - base and both clamps are exact, the two subtractions have the same real result, and each
// is rounded once.  voxel and base are 16-bit values; the bound on the window keeps every intermediate inside +-2^24.
// false: the kernel adds the base back as an integer before the convert.
inline bool streamBaseFoldsIntoWindow(int min_val, int max_val, int base)
{
    const int lim = (1 << 24) - (1 << 17);
    return base >= 0 && base < (1 << 16) && min_val > -lim && min_val < lim && max_val > -lim && max_val < lim;
}

}  // namespace vr
