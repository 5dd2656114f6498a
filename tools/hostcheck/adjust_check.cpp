// Host-only check of csrc/adjust_core.h: the cut / lo / hi / LUT arithmetic of the contrast adjustment and the descriptor validation of
// surya_rec_adjust_contrast: no GPU, no HIP call, plain C++. Meant to run under the host sanitizers:
//
//   clang++ -std=c++17 -O1 -g -Iinclude -fsanitize=address,undefined tools/hostcheck/adjust_check.cpp -o /tmp/adjust_check && /tmp/adjust_check
//
// The scanned form of the bounds (what the 256 lanes evaluate) is held to the serial form (Pillow's loops) on random and hand-made
// histograms; LUT values and validation verdicts are written out by hand below.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../surya_amd/csrc/adjust_core.h"

using namespace sa::adjust;

static int failures = 0;
#define CHECK(cond) \
    do { if (!(cond)) { ++failures; std::printf("FAILED line %d: %s\n", __LINE__, #cond); } } while (0)

static uint32_t rnd_state = 12345u;
static uint32_t rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }

static void same_bounds(const uint32_t* h, int c) {
    int a, b, x, y;
    bounds_serial(h, c, &a, &b);
    bounds_scanned(h, c, &x, &y);
    CHECK(a == x && b == y);
}

static AdjustDesc desc(long src_off, int sw, int sh, int x0, int y0, int w, int h, int cutoff, long out_off) {
    AdjustDesc d;
    std::memset(&d, 0, sizeof d);
    d.src_off = src_off; d.src_w = sw; d.src_h = sh; d.x0 = x0; d.y0 = y0; d.w = w; d.h = h; d.cutoff = cutoff; d.out_off = out_off;
    return d;
}

int main() {
    // luma and the cut
    CHECK(luma(0, 0, 0) == 0 && luma(255, 255, 255) == 255 && luma(255, 0, 0) == 76 && luma(0, 255, 0) == 150 && luma(0, 0, 255) == 29);
    CHECK(cut_count(0, 49) == 0 && cut_count(3, 49) == 1 && cut_count(2, 49) == 0 && cut_count(100, 1) == 1);
    CHECK(cut_count(4294967295u, 49) == 2104533974u);                      // n * 49 needs more than 32 bits
    CHECK(bin_left(5, 0, 0) == 5 && bin_left(5, 3, 0) == 2 && bin_left(5, 7, 0) == 0 && bin_left(5, 7, 4) == 2 && bin_left(5, 7, 9) == 5);
    // the LUT: the identity when hi <= lo; lut[hi] = 254 for (0, 25); the ends
    for (int i = 0; i < 256; ++i) CHECK(lut_entry(i, 7, 7) == i && lut_entry(i, 255, 0) == i);
    CHECK(lut_entry(25, 0, 25) == 254 && lut_entry(0, 0, 25) == 0 && lut_entry(26, 0, 25) == 255 && lut_entry(255, 0, 25) == 255);
    CHECK(lut_entry(255, 0, 255) == 255 && lut_entry(128, 0, 255) == 128 && lut_entry(10, 20, 30) == 0 && lut_entry(25, 20, 30) == 127);
    int short_of_255 = 0;
    for (int lo = 0; lo < 256; ++lo)
        for (int hi = lo + 1; hi < 256; ++hi) {
            short_of_255 += lut_entry(hi, lo, hi) == 254;
            CHECK(lut_entry(lo, lo, hi) == 0 && lut_entry(hi, lo, hi) >= 254);
            for (int i = 1; i < 256; ++i) CHECK(lut_entry(i, lo, hi) >= lut_entry(i - 1, lo, hi));
        }
    CHECK(short_of_255 == 4852);
    // bounds: empty, one bin, two levels, random
    uint32_t h[256];
    std::memset(h, 0, sizeof h);
    int lo, hi;
    bounds_serial(h, 10, &lo, &hi);
    CHECK(lo == 255 && hi == 0);
    same_bounds(h, 10);
    h[255] = 9;
    bounds_serial(h, 49, &lo, &hi);
    CHECK(lo == 255 && hi == 255);
    same_bounds(h, 49);
    h[3] = 1; h[255] = 99;                                                // 100 pixels, 1 %: the dark one goes, then one bright one
    bounds_serial(h, 1, &lo, &hi);
    CHECK(lo == 255 && hi == 255);
    same_bounds(h, 1);
    bounds_serial(h, 0, &lo, &hi);
    CHECK(lo == 3 && hi == 255);
    for (int t = 0; t < 4000; ++t) {
        const int bins = 1 + (int)(rnd() % 256), scale = 1 + (int)(rnd() % 1000);
        std::memset(h, 0, sizeof h);
        for (int k = 0; k < bins; ++k) h[rnd() % 256] += rnd() % (uint32_t)scale;
        for (int c : {0, 1, 10, 25, 49}) same_bounds(h, c);
    }
    std::memset(h, 0, sizeof h);
    h[0] = 4000000000u; h[200] = 200000000u;                              // a sum beyond 2^32 cannot come from a validated crop; just below it can
    same_bounds(h, 49);

    // descriptor validation: pages at P, outputs at O (pages' own allocation, behind a 100 x 50 RGB page)
    const uintptr_t P = 0x10000000u;
    std::vector<AdjustDesc> d = {desc(0, 100, 50, 10, 5, 20, 10, 2, 15000), desc(0, 100, 50, 80, 40, 20, 10, 0, 15600)};
    CHECK(validate(d.data(), 2, P, P, false, 3) == 0);
    CHECK(validate(d.data(), 0, P, P, false, 3) == 0 && validate(d.data(), -1, P, P, false, 3) == 1);
    CHECK(validate(d.data(), 2, P, P, false, 5) == 1 && validate(nullptr, 2, P, P, false, 3) == 1 && validate(d.data(), 2, 0, P, false, 3) == 1);
    auto bad = [&](int i, void (*edit)(AdjustDesc&), int pix = 3, bool mask = false) {
        std::vector<AdjustDesc> e = d;
        edit(e[i]);
        return validate(e.data(), 2, P, P, mask, pix);
    };
    CHECK(bad(0, [](AdjustDesc& e) { e.w = 0; }) == 1);
    CHECK(bad(0, [](AdjustDesc& e) { e.h = -1; }) == 1);
    CHECK(bad(0, [](AdjustDesc& e) { e.x0 = -1; }) == 1);
    CHECK(bad(1, [](AdjustDesc& e) { e.x0 = 81; }) == 1);                 // one pixel over the right edge
    CHECK(bad(1, [](AdjustDesc& e) { e.y0 = 41; }) == 1);
    CHECK(bad(0, [](AdjustDesc& e) { e.cutoff = 50; }) == 1);
    CHECK(bad(0, [](AdjustDesc& e) { e.cutoff = -1; }) == 1);
    CHECK(bad(0, [](AdjustDesc& e) { e.cutoff = 49; }) == 0);
    CHECK(bad(0, [](AdjustDesc& e) { e.out_off = -4; }) == 1);
    CHECK(bad(0, [](AdjustDesc& e) { e.out_off = 14999; }) == 1);         // its first byte is the page's last
    CHECK(bad(0, [](AdjustDesc& e) { e.out_off = 15001; }) == 1);         // its last byte is the other output's first
    CHECK(bad(1, [](AdjustDesc& e) { e.out_off = 15599; }) == 1);
    CHECK(bad(1, [](AdjustDesc& e) { e.out_off = 15000; }) == 1);         // the same range twice
    CHECK(bad(0, [](AdjustDesc& e) { e.has_poly = 1; }) == 1);            // no mask arena
    CHECK(bad(0, [](AdjustDesc& e) { e.has_poly = 1; }, 3, true) == 0);
    CHECK(bad(0, [](AdjustDesc& e) { e.has_poly = 2; }, 3, true) == 1);
    CHECK(bad(0, [](AdjustDesc& e) { e.has_poly = 1; e.mask_off = -1; }, 3, true) == 1);
    CHECK(bad(0, [](AdjustDesc& e) { e.w = 100; e.x0 = 0; e.h = 50; e.y0 = 0; e.src_w = 1 << 15; e.src_h = 1 << 15; e.w = 1 << 15; e.h = (1 << 13) + 1; }) == 1);
    {   // two masks on the same bytes
        std::vector<AdjustDesc> e = d;
        e[0].has_poly = e[1].has_poly = 1; e[0].mask_off = 0; e[1].mask_off = 199;
        CHECK(validate(e.data(), 2, P, P, true, 3) == 1);
        e[1].mask_off = 200;
        CHECK(validate(e.data(), 2, P, P, true, 3) == 0);
    }
    {   // 4-byte pixels: every offset a multiple of 4, and the pointers too
        std::vector<AdjustDesc> e = {desc(0, 100, 50, 10, 5, 20, 10, 2, 20000), desc(0, 100, 50, 80, 40, 20, 10, 0, 20800)};
        CHECK(validate(e.data(), 2, P, P, false, 4) == 0);
        CHECK(validate(e.data(), 2, P + 2, P, false, 4) == 1 && validate(e.data(), 2, P, P + 1, false, 4) == 1);
        e[1].out_off = 20802;
        CHECK(validate(e.data(), 2, P, P, false, 4) == 1);
        e[1].out_off = 20800; e[1].src_off = 2;
        CHECK(validate(e.data(), 2, P, P, false, 4) == 1);
    }
    {   // a rectified-then-adjusted line: its source is a crop behind the pages, its output lies behind that
        std::vector<AdjustDesc> e = {desc(15000, 20, 10, 0, 0, 20, 10, 2, 15600)};
        CHECK(validate(e.data(), 1, P, P, false, 3) == 0);
        e[0].out_off = 15596;
        CHECK(validate(e.data(), 1, P, P, false, 3) == 1);
    }
    {   // outputs in an allocation of their own may use the offsets the pages use
        CHECK(validate(d.data(), 2, P, P + 0x1000000u, false, 3) == 0);
        std::vector<AdjustDesc> e = d;
        e[0].out_off = 0; e[1].out_off = 600;
        CHECK(validate(e.data(), 2, P, P + 0x1000000u, false, 3) == 0 && validate(e.data(), 2, P, P, false, 3) == 1);
    }
    std::printf(failures ? "adjust_check: %d FAILED\n" : "adjust_check: all passed\n", failures);
    return failures ? 1 : 0;
}
