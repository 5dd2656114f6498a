// The integer and float64 arithmetic of the contrast adjustment (rec_adjust.h), host and device: Pillow's ImageOps.autocontrast with
// preserve_tone, restated. The kernels and the plain C++ host check (tools/hostcheck/adjust_check.cpp) compile these same functions.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SA_ADJ_HD __host__ __device__ inline
#else
#define SA_ADJ_HD inline
#endif

namespace sa {
namespace adjust {

// Pillow's convert("L"): ITU-R 601-2 luma in 16-bit fixed point, rounded
SA_ADJ_HD unsigned luma(unsigned r, unsigned g, unsigned b) { return (19595u * r + 38470u * g + 7471u * b + 32768u) >> 16; }

// n * cutoff // 100 for n counted pixels: 64-bit, so that a whole-page crop (n < 2^32) cannot overflow
SA_ADJ_HD uint32_t cut_count(uint32_t n, int cutoff) { return (uint32_t)((uint64_t)n * (uint64_t)cutoff / 100u); }

// What is left of a bin of `h` counts after `cut` counts were removed from one end of the histogram, `before` of them lying in front
// of this bin on that end (Pillow's loop: empty bins while cut exceeds them, then take the rest from the first bin that holds it)
SA_ADJ_HD uint32_t bin_left(uint32_t h, uint32_t cut, uint32_t before) {
    const uint32_t take = cut > before ? cut - before : 0u;
    return h - (take < h ? take : h);
}

// lut[i] for bounds lo < hi: int(i * scale + offset) clamped, scale = 255.0 / (hi - lo), offset = -lo * scale; one division, one
// multiply, one add in float64, never contracted (for 4852 of the 32 640 pairs lut[hi] is 254: (0, 25) is one)
SA_ADJ_HD int lut_entry(int i, int lo, int hi) {
#pragma clang fp contract(off)
    if (hi <= lo) return i;
    const double scale = 255.0 / (double)(hi - lo);
    const double offset = (double)(-lo) * scale;
    const double v = (double)i * scale + offset;
    const int r = (int)v;                                     // |v| <= 255 * 255: in range; truncation toward zero like Python's int()
    return r < 0 ? 0 : (r > 255 ? 255 : r);
}

// The bounds of a 256-bin histogram, serially, as Pillow's loops run: the reference the device's scans are checked against on the host
inline void bounds_serial(const uint32_t* hist, int cutoff, int* lo_out, int* hi_out) {
    uint32_t h[256];
    uint64_t n = 0;
    for (int i = 0; i < 256; ++i) { h[i] = hist[i]; n += hist[i]; }
    if (cutoff) {
        uint64_t cut = n * (uint64_t)cutoff / 100u;
        for (int lo = 0; lo < 256; ++lo) {
            if (cut > h[lo]) { cut -= h[lo]; h[lo] = 0; } else { h[lo] -= (uint32_t)cut; cut = 0; }
            if (cut == 0) break;
        }
        cut = n * (uint64_t)cutoff / 100u;
        for (int hi = 255; hi >= 0; --hi) {
            if (cut > h[hi]) { cut -= h[hi]; h[hi] = 0; } else { h[hi] -= (uint32_t)cut; cut = 0; }
            if (cut == 0) break;
        }
    }
    int lo = 0, hi = 255;
    for (lo = 0; lo < 255; ++lo) if (h[lo]) break;           // (an empty histogram leaves lo = 255, hi = 0: the identity)
    for (hi = 255; hi > 0; --hi) if (h[hi]) break;
    *lo_out = lo; *hi_out = hi;
}

// The same bounds by the formulas the 256 lanes evaluate (bin_left over an exclusive prefix, then over an exclusive suffix)
inline void bounds_scanned(const uint32_t* hist, int cutoff, int* lo_out, int* hi_out) {
    uint32_t r[256], n = 0, run = 0;
    for (int i = 0; i < 256; ++i) n += hist[i];
    const uint32_t cut = cut_count(n, cutoff);
    for (int i = 0; i < 256; ++i) { r[i] = bin_left(hist[i], cut, run); run += hist[i]; }
    run = 0;
    for (int i = 255; i >= 0; --i) { const uint32_t left = bin_left(r[i], cut, run); run += r[i]; r[i] = left; }
    int lo = 255, hi = 0;
    for (int i = 0; i < 256; ++i) if (r[i]) { lo = i < lo ? i : lo; hi = i > hi ? i : hi; }
    *lo_out = lo; *hi_out = hi;
}

// ------------------------------------------------------------------------------------------------------------ descriptors
struct AdjustDesc {
    long src_off;                // byte offset of the source page's first pixel in `pages` (a page, or a rectified crop as a page of its own)
    int src_w, src_h;
    int x0, y0, w, h;            // crop rectangle inside the source (w, h >= 1)
    int cutoff;                  // integer percent, 0..49
    int has_poly;                // 1: the histogram counts the polygon's pixels only, the others read as 255 before the LUT
    float poly[8];               // 4 (x, y) vertices relative to the crop origin (LineDesc::poly)
    long out_off;                // byte offset of the adjusted crop's first pixel in `out`: [h][w][pixel_stride]
    long mask_off;               // byte offset of the line's [h][w] mask in the mask arena (has_poly)
};

static_assert(sizeof(AdjustDesc) == 88, "AdjustDesc layout is part of the C ABI (include/surya_amd.h, preprocess_gpu.py)");

constexpr long ADJUST_MAX_PIXELS = 1L << 28;                  // per crop: pixel and byte indices inside a crop stay 32-bit

// Every check of surya_rec_adjust_contrast on its HOST descriptor array, with no device in sight: 0 = all pass. `pages_addr`, `out_addr`:
// the two device pointers as integers (ranges are compared as absolute addresses, so `out` may or may not lie in the pages' allocation).
inline int validate(const AdjustDesc* d, int n, uintptr_t pages_addr, uintptr_t out_addr, bool have_mask, int pix) {
    if (n < 0 || (pix != 3 && pix != 4)) return 1;
    if (n == 0) return 0;
    if (!d || !pages_addr || !out_addr) return 1;
    if (pix == 4 && ((pages_addr | out_addr) & 3)) return 1;
    struct Range { uintptr_t a, b; };
    Range* outs = new Range[n];
    Range* masks = new Range[n];
    int nm = 0, bad = 0;
    for (int i = 0; i < n && !bad; ++i) {
        const AdjustDesc& e = d[i];
        if (e.src_w <= 0 || e.src_h <= 0 || e.w <= 0 || e.h <= 0 || e.x0 < 0 || e.y0 < 0) bad = 1;
        else if (e.x0 > e.src_w - e.w || e.y0 > e.src_h - e.h) bad = 1;                 // the crop lies inside its source
        else if ((long)e.w * e.h > ADJUST_MAX_PIXELS) bad = 1;
        else if (e.cutoff < 0 || e.cutoff > 49) bad = 1;
        else if (e.src_off < 0 || e.out_off < 0) bad = 1;
        else if (pix == 4 && ((e.src_off | e.out_off) & 3)) bad = 1;
        else if (e.has_poly != 0 && e.has_poly != 1) bad = 1;
        else if (e.has_poly && (!have_mask || e.mask_off < 0)) bad = 1;
        if (bad) break;
        outs[i].a = out_addr + (uintptr_t)e.out_off;
        outs[i].b = outs[i].a + (uintptr_t)e.w * e.h * pix;
        if (e.has_poly) { masks[nm].a = (uintptr_t)e.mask_off; masks[nm].b = masks[nm].a + (uintptr_t)e.w * e.h; ++nm; }
    }
    auto by_start = [](const void* x, const void* y) {
        const uintptr_t a = static_cast<const Range*>(x)->a, b = static_cast<const Range*>(y)->a;
        return a < b ? -1 : (a > b ? 1 : 0);
    };
    if (!bad) {
        qsort(outs, n, sizeof(Range), by_start);
        qsort(masks, nm, sizeof(Range), by_start);
        for (int i = 1; i < n && !bad; ++i) bad = outs[i].a < outs[i - 1].b;            // outputs against each other
        for (int i = 1; i < nm && !bad; ++i) bad = masks[i].a < masks[i - 1].b;         // masks against each other
    }
    for (int i = 0; i < n && !bad; ++i) {                                                // every source page against the outputs
        const uintptr_t a = pages_addr + (uintptr_t)d[i].src_off, b = a + (uintptr_t)d[i].src_w * d[i].src_h * pix;
        int lo = 0, hi = n;                                                              // first output whose end lies behind a
        while (lo < hi) { const int m = (lo + hi) / 2; if (outs[m].b > a) hi = m; else lo = m + 1; }
        bad = lo < n && outs[lo].a < b;
    }
    delete[] outs;
    delete[] masks;
    return bad;
}

}  // namespace adjust
}  // namespace sa
