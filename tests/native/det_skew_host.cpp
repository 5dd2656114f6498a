// Host build of csrc/det_skew_core.h, the bin arithmetic the kernels of csrc/det_skew.h run: det_skew_host() computes the scores of one
// map the way the two kernels do (compact the text pixels into a packed list, histogram per angle, squared differences in uint64) and is
// what tests/test_det_skew_cpu.py holds to the numpy reference (surya_amd/detection/skew.py). No GPU, no HIP call, plain C++.
//
// The file is also a program of its own, meant to run under the host sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tests/native/det_skew_host.cpp -o det_skew_host && ./det_skew_host
//
// main() checks the int32 and bin bounds at the largest sizes, hand-made profiles, and that a table outside the contract only ever
// produces bins the caller drops.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../surya_amd/csrc/det_skew_core.h"

using namespace sa::skew;

extern "C" int det_skew_host(const float* heat, int H, int W, float threshold, const int32_t* cs, int n_angles, uint64_t* scores,
                             int32_t* n_text) {
    if (!heat || !cs || !scores || !n_text || H <= 0 || W <= 0 || n_angles < 1 || n_angles > SKEW_MAX_ANGLES || !(threshold >= 0.f)) return -1;
    if (H > SKEW_MAX_DIM || W > SKEW_MAX_DIM) return -2;
    std::vector<uint32_t> list;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            if (skew_is_text(heat[(size_t)y * W + x], threshold)) list.push_back(skew_pack(x, y));
    *n_text = (int32_t)list.size();
    const int nb = H + W;
    std::vector<uint32_t> hist((size_t)nb);
    for (int a = 0; a < n_angles; ++a) {
        const int c = cs[2 * a], s = cs[2 * a + 1], off = skew_offset(W, s);
        std::fill(hist.begin(), hist.end(), 0u);
        for (uint32_t p : list) {
            const int r = skew_bin(skew_packed_x(p), skew_packed_y(p), c, s, off);
            if ((unsigned)r < (unsigned)nb) ++hist[(size_t)r];
        }
        uint64_t acc = 0;
        for (int r = 0; r + 1 < nb; ++r) acc += skew_sqdiff(hist[(size_t)r + 1], hist[(size_t)r]);
        scores[a] = acc;
    }
    return 0;
}

static int failures = 0;
#define CHECK(cond) \
    do { if (!(cond)) { ++failures; std::printf("FAILED line %d: %s\n", __LINE__, #cond); } } while (0)

static void coeff(double deg, int* c, int* s) {
    const double t = deg * 3.14159265358979323846 / 180.0;
    *c = (int)std::nearbyint(std::cos(t) * 65536.0);
    *s = (int)std::nearbyint(std::sin(t) * 65536.0);
}

int main() {
    // the four corners of the largest maps stay inside [0, H + W) and inside int32 for every angle of the contract
    const int shapes[][2] = {{8192, 8192}, {8, 8192}, {8192, 8}, {1, 1}, {300, 7}};
    for (auto& hw : shapes) {
        const int H = hw[0], W = hw[1], nb = H + W;
        for (double deg = -45.0; deg <= 45.0; deg += 0.25) {
            int c, s;
            coeff(deg, &c, &s);
            CHECK(c > 0 && std::abs(s) <= c);
            const int off = skew_offset(W, s);
            const int xs[2] = {0, W - 1}, ys[2] = {0, H - 1};
            int lo = nb, hi = -1;
            for (int x : xs)
                for (int y : ys) {
                    const long long exact = ((long long)y * c - (long long)x * s + (long long)(W - 1) * (s > 0 ? s : 0));
                    CHECK(exact >= 0 && exact < (1ll << 31));
                    const int r = skew_bin(x, y, c, s, off);
                    CHECK(r == (int)(exact >> 16));
                    lo = r < lo ? r : lo;
                    hi = r > hi ? r : hi;
                }
            CHECK(lo == 0 && hi < nb);
        }
    }
    // packing
    CHECK(skew_packed_x(skew_pack(8191, 8191)) == 8191 && skew_packed_y(skew_pack(8191, 8191)) == 8191 && skew_pack(3, 2) == 0x20003u);
    CHECK(skew_sqdiff(0u, 4000000000u) == 16000000000000000000ull && skew_sqdiff(7u, 7u) == 0);
    // a hand-made profile: two full rows of a 4 x 8 map at 0 degrees -> P = (0, 8, 0, 8, 0 ...), four steps of 8
    {
        std::vector<float> m(4 * 8, 0.f);
        for (int x = 0; x < 8; ++x) m[1 * 8 + x] = m[3 * 8 + x] = 1.f;
        const int32_t cs[6] = {65536, 0, 46341, 46341, 46341, -46341};
        uint64_t sc[3];
        int32_t n = -1;
        CHECK(det_skew_host(m.data(), 4, 8, 0.5f, cs, 3, sc, &n) == 0 && n == 16 && sc[0] == 4 * 64);
        CHECK(sc[1] == sc[2]);                                   // the two rows are symmetric under a left-right flip
        m[0] = 0.5f;                                             // a value AT the threshold is not text
        CHECK(det_skew_host(m.data(), 4, 8, 0.5f, cs, 3, sc, &n) == 0 && n == 16);
        CHECK(det_skew_host(m.data(), 4, 8, -0.f, cs, 3, sc, &n) == 0 && n == 17);
        CHECK(det_skew_host(m.data(), 4, 8, -1.f, cs, 3, sc, &n) == -1 && det_skew_host(m.data(), 4, 8, NAN, cs, 3, sc, &n) == -1);
        CHECK(det_skew_host(m.data(), 4, 8, 0.5f, cs, 0, sc, &n) == -1 && det_skew_host(m.data(), 4, 8, 0.5f, cs, 1025, sc, &n) == -1);
    }
    // tables outside the contract: whatever the words are, a bin is either dropped or inside the histogram (no signed overflow: the
    // products wrap as unsigned words, which the undefined-behaviour sanitizer would report otherwise)
    {
        std::vector<float> m(16 * 16, 1.f);
        uint32_t st = 99u;
        for (int k = 0; k < 200; ++k) {
            int32_t cs[2];
            st = st * 1664525u + 1013904223u; cs[0] = (int32_t)st;
            st = st * 1664525u + 1013904223u; cs[1] = (int32_t)st;
            if (k == 0) { cs[0] = INT32_MIN; cs[1] = INT32_MIN; }
            if (k == 1) { cs[0] = INT32_MAX; cs[1] = INT32_MAX; }
            uint64_t sc;
            int32_t n;
            CHECK(det_skew_host(m.data(), 16, 16, 0.f, cs, 1, &sc, &n) == 0 && n == 256);
        }
    }
    // all text and no text
    {
        std::vector<float> m(12 * 20, 1.f), z(12 * 20, 0.f);
        const int32_t cs[2] = {65536, 0};
        uint64_t sc;
        int32_t n;
        CHECK(det_skew_host(m.data(), 12, 20, 0.f, cs, 1, &sc, &n) == 0 && n == 240 && sc == 400);      // one step down behind row 11
        CHECK(det_skew_host(z.data(), 12, 20, 0.f, cs, 1, &sc, &n) == 0 && n == 0 && sc == 0);
    }
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("det_skew_host: all checks passed\n");
    return 0;
}
