// Host build of csrc/det_centerline_core.h, the bin arithmetic the kernels of csrc/det_centerline.h run: det_centerline_host() computes the
// profiles of one page the way the two kernels do (empty bins and axes first, then one raster sweep: label -> root -> compact index -> box
// -> bin) and is what tests/test_det_centerline_cpu.py holds to the numpy reference (surya_amd/detection/centerline.py). No GPU, no HIP
// call, plain C++.
//
// The file is also a program of its own, meant to run under the host sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tests/native/det_centerline_host.cpp -o det_centerline_host && ./det_centerline_host
//
// main() checks the bin rule at the largest extent, the axis tie, the run sums, hand-made pages and that a workspace full of nonsense is
// read without a step out of bounds.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../surya_amd/csrc/det_post_core.h"
#include "../../surya_amd/csrc/det_centerline_core.h"

using namespace sa::centerline;
using sa::post::CompStats;

// label: [H * W] the root's raster index, -1 = background; area: [H * W], at a root its compact index or -1; comp: [max_boxes];
// count: the page's kept components, -1 = the page overflowed. Outputs: [max_boxes][knots] and [max_boxes].
extern "C" int det_centerline_host(const int32_t* label, const int32_t* area, const CompStats* comp, int count, int H, int W, int max_boxes,
                                   int knots, uint32_t* cnt, uint64_t* sum, int32_t* lo, int32_t* hi, int32_t* axis) {
    if (!label || !area || !comp || !cnt || !sum || !lo || !hi || !axis) return -1;
    if (H <= 0 || W <= 0 || max_boxes <= 0 || knots < CL_MIN_KNOTS || knots > CL_MAX_KNOTS) return -1;
    if (H > CL_MAX_DIM || W > CL_MAX_DIM) return -2;
    const int n_sel = count < 0 ? 0 : (count > max_boxes ? max_boxes : count);
    for (long j = 0; j < (long)max_boxes * knots; ++j) { cnt[j] = 0; sum[j] = 0; lo[j] = CL_EMPTY_LO; hi[j] = CL_EMPTY_HI; }
    for (int c = 0; c < max_boxes; ++c) axis[c] = c < n_sel ? cl_axis(comp[c].x0, comp[c].x1, comp[c].y0, comp[c].y1) : -1;
    const long N = (long)H * W;
    for (long i = 0; i < N; ++i) {
        const int r = label[i];
        if (r < 0 || r >= N) continue;
        const int idx = area[r];
        if (idx < 0 || idx >= n_sel) continue;
        const ClFrame f = cl_frame(comp[idx].x0, comp[idx].x1, comp[idx].y0, comp[idx].y1);
        const int x = (int)(i % W), y = (int)(i / W);
        const int k = cl_bin(f, f.axis == 0 ? x : y, knots);
        if (k < 0) continue;
        const int p = f.axis == 0 ? y : x;
        const long o = (long)idx * knots + k;
        ++cnt[o]; sum[o] += (uint64_t)p;
        lo[o] = p < lo[o] ? p : lo[o];
        hi[o] = p > hi[o] ? p : hi[o];
    }
    return 0;
}

static int failures = 0;
#define CHECK(cond) \
    do { if (!(cond)) { ++failures; std::printf("FAILED line %d: %s\n", __LINE__, #cond); } } while (0)

int main() {
    // the bin rule: first and last column of every extent land in the first and last bin, bins never decrease, none beyond knots - 1
    for (int extent : {1, 2, 3, 15, 16, 17, 63, 64, 65, 1000, 8191, 8192})
        for (int knots : {2, 3, 16, 63, 64}) {
            const ClFrame f{0, 100, extent};
            int prev = 0;
            CHECK(cl_bin(f, 100, knots) == 0 && cl_bin(f, 100 + extent - 1, knots) == (int)(((long)(extent - 1) * knots) / extent));
            CHECK(cl_bin(f, 99, knots) == -1 && cl_bin(f, 100 + extent, knots) == -1);
            for (int t = 0; t < extent; ++t) {
                const int k = cl_bin(f, 100 + t, knots);
                CHECK(k == (int)(((long)t * knots) / extent) && k >= prev && k < knots);
                prev = k;
            }
        }
    // axis: a tie is horizontal
    CHECK(cl_axis(3, 9, 10, 16) == 0 && cl_axis(3, 9, 10, 17) == 1 && cl_axis(3, 10, 10, 16) == 0 && cl_axis(0, 0, 0, 0) == 0);
    CHECK(cl_frame(3, 9, 10, 17).origin == 10 && cl_frame(3, 9, 10, 17).extent == 8 && cl_frame(3, 9, 10, 16).extent == 7);
    // the sum of a run of consecutive coordinates
    CHECK(cl_arith_sum(5, 1) == 5 && cl_arith_sum(5, 4) == 26 && cl_arith_sum(0, 256) == 32640 && cl_arith_sum(8188, 4) == 32758);
    // a hand-made page: one 2 x 12 bar (rows 3, 4, columns 2 .. 13) and one 12 x 2 bar (columns 16, 17, rows 2 .. 13) on 16 x 20
    {
        const int H = 16, W = 20, MB = 4, K = 4;
        std::vector<int32_t> label(H * W, -1), area(H * W, 0x5a5a5a5a);
        std::vector<CompStats> comp(MB);
        const int root_a = 2 * W + 16, root_b = 3 * W + 2;       // raster order: the vertical bar starts first
        for (int y = 2; y <= 13; ++y) for (int x = 16; x <= 17; ++x) label[y * W + x] = root_a;
        for (int y = 3; y <= 4; ++y) for (int x = 2; x <= 13; ++x) label[y * W + x] = root_b;
        area[root_a] = 0; area[root_b] = 1;
        comp[0] = CompStats{16, 17, 2, 13, 24, 0.9f};
        comp[1] = CompStats{2, 13, 3, 4, 24, 0.9f};
        std::vector<uint32_t> cnt(MB * K, 77);
        std::vector<uint64_t> sum(MB * K, 77);
        std::vector<int32_t> lo(MB * K, 77), hi(MB * K, 77), axis(MB, 77);
        CHECK(det_centerline_host(label.data(), area.data(), comp.data(), 2, H, W, MB, K, cnt.data(), sum.data(), lo.data(), hi.data(), axis.data()) == 0);
        CHECK(axis[0] == 1 && axis[1] == 0 && axis[2] == -1 && axis[3] == -1);
        for (int k = 0; k < K; ++k) {
            CHECK(cnt[k] == 6 && sum[k] == 3 * (16 + 17) && lo[k] == 16 && hi[k] == 17);                    // three rows of two pixels, p = x
            CHECK(cnt[K + k] == 6 && sum[K + k] == 3 * (3 + 4) && lo[K + k] == 3 && hi[K + k] == 4);        // three columns of two pixels, p = y
            CHECK(cnt[2 * K + k] == 0 && sum[2 * K + k] == 0 && lo[2 * K + k] == CL_EMPTY_LO && hi[2 * K + k] == CL_EMPTY_HI);
        }
        // an overflowed page: nothing is counted
        CHECK(det_centerline_host(label.data(), area.data(), comp.data(), -1, H, W, MB, K, cnt.data(), sum.data(), lo.data(), hi.data(), axis.data()) == 0);
        CHECK(axis[0] == -1 && cnt[0] == 0 && lo[0] == CL_EMPTY_LO);
        // refusals
        CHECK(det_centerline_host(label.data(), area.data(), comp.data(), 2, H, W, MB, 1, cnt.data(), sum.data(), lo.data(), hi.data(), axis.data()) == -1);
        CHECK(det_centerline_host(label.data(), area.data(), comp.data(), 2, H, W, MB, 65, cnt.data(), sum.data(), lo.data(), hi.data(), axis.data()) == -1);
        CHECK(det_centerline_host(nullptr, area.data(), comp.data(), 2, H, W, MB, K, cnt.data(), sum.data(), lo.data(), hi.data(), axis.data()) == -1);
    }
    // a workspace full of nonsense: labels, indices and boxes from a generator; every read and write stays inside the arrays
    {
        const int H = 24, W = 36, MB = 8, K = 5;
        std::vector<int32_t> label(H * W), area(H * W);
        std::vector<CompStats> comp(MB);
        uint32_t st = 7u;
        auto next = [&]() { st = st * 1664525u + 1013904223u; return (int32_t)st; };
        for (int round = 0; round < 50; ++round) {
            for (auto& v : label) v = round % 2 ? next() : next() % (2 * H * W);
            for (auto& v : area) v = round % 3 ? next() % 16 : next();
            for (auto& c : comp) c = CompStats{next() % 64, next() % 64, next() % 64, next() % 64, next(), 0.f};
            if (round < 4) for (auto& c : comp) c = CompStats{next(), next(), next(), next(), next(), 0.f};
            std::vector<uint32_t> cnt(MB * K);
            std::vector<uint64_t> sum(MB * K);
            std::vector<int32_t> lo(MB * K), hi(MB * K), axis(MB);
            CHECK(det_centerline_host(label.data(), area.data(), comp.data(), round % 12, H, W, MB, K, cnt.data(), sum.data(), lo.data(), hi.data(),
                                      axis.data()) == 0);
        }
    }
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("det_centerline_host: all checks passed\n");
    return 0;
}
