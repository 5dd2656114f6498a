// Page skew from the heat map: the integer arithmetic of the projection profile, shared by the HIP kernels (det_skew.h) and a plain-C++
// build (tests/native/det_skew_host.cpp). surya_amd/detection/skew.py states the whole rule; this is its per-pixel and per-bin half.
//
//   text      heat > threshold (strict, as the labelling of det_post.h; threshold >= 0, so zero pad columns never count)
//   bin       r = (y * c - x * s + off) >> 16, off = (W - 1) * max(s, 0), with c = rint(cos * 65536), s = rint(sin * 65536) made on the
//             host: no trigonometry and no floating-point product here, so every machine gives the same bits. For c > 0, |s| <= c and
//             H, W <= 8192 the value stays below 2^31 and r lies in [0, H + W). The products are formed as unsigned words, so a table
//             that breaks those bounds wraps instead of overflowing; its bins are then meaningless and the CALLER of skew_bin drops
//             every r outside [0, H + W).
//   score     sum over r of (P[r + 1] - P[r])^2 in 64-bit integers: independent of the order of the sum.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SA_SKEW_HD __host__ __device__ __forceinline__
#else
#define SA_SKEW_HD inline
#endif

namespace sa {
namespace skew {

constexpr int SKEW_MAX_DIM = 8192;        // height and width limit: keeps the bin arithmetic inside int32 and (y << 16) | x inside a word
constexpr int SKEW_MAX_ANGLES = 1024;
constexpr int SKEW_FRAC_BITS = 16;

SA_SKEW_HD bool skew_is_text(float heat, float threshold) { return heat > threshold; }

SA_SKEW_HD int skew_offset(int W, int s) { return (int)((uint32_t)(W - 1) * (uint32_t)(s > 0 ? s : 0)); }

SA_SKEW_HD int skew_bin(int x, int y, int c, int s, int off) {
    const uint32_t v = (uint32_t)y * (uint32_t)c - (uint32_t)x * (uint32_t)s + (uint32_t)off;
    return (int)v >> SKEW_FRAC_BITS;                              // arithmetic shift: floor for negative values
}

SA_SKEW_HD uint32_t skew_pack(int x, int y) { return ((uint32_t)y << 16) | (uint32_t)x; }
SA_SKEW_HD int skew_packed_x(uint32_t p) { return (int)(p & 0xffffu); }
SA_SKEW_HD int skew_packed_y(uint32_t p) { return (int)(p >> 16); }

SA_SKEW_HD uint64_t skew_sqdiff(uint32_t a, uint32_t b) {
    const uint64_t d = a > b ? (uint64_t)a - b : (uint64_t)b - a;       // < 2^32: the square fits 64 bits
    return d * d;
}

}  // namespace skew
}  // namespace sa
