// Rectification of rotated line quadrilaterals ON THE DEVICE: page pixels -> upright uint8 crops, written behind the pages as
// small synthetic "pages" that the line pre-processing (rec_prep.h) then reads like any other page through
// (page_off, page_w, x0 = y0 = 0) -- LineDesc and the four prep kernels do not change.
//
// The rule is warp_quad of surya_amd/common/imageops.py, restated per pixel: output pixel (u, v) samples the page at the image of
// (u + 0.5, v + 0.5) under the quad's homography, minus 0.5 on both axes; 4 x 4 Keys cubic taps (a = -0.75) around floor() of that
// point, tap indices clamped to the page (replicate border); float64 products summed in tap order without FMA contraction, the
// horizontal pass per tap row first, then the vertical taps; rint (half to even), clamp to 0..255. With 4-byte pixels X is 0.
//
// Gather work served from L1 / L2 (a page is 3-8 MB, neighbouring output pixels share 12 of their 16 taps): one thread per output
// pixel, 16 x 16 pixel workgroups so that a rotated footprint stays a compact patch of the page, no LDS. Descriptors travel in
// the kernel-argument segment (wave-uniform: the homography sits in scalar registers), RECTIFY_BATCH lines per launch.
#pragma once
#include "common.h"
#include "cv_resample.h"

namespace sa {
namespace prep {

struct RectifyDesc {
    long page_off;               // byte offset of the source page's first pixel in `pages`
    int page_w, page_h;
    int out_w, out_h;            // size of the rectified crop (quad_size)
    long out_off;                // byte offset of the crop's first pixel in `out`
    double h[9];                 // row-major homography: crop rectangle (grid-line coordinates) -> page, h[8] = 1
};

static_assert(sizeof(RectifyDesc) == 104, "RectifyDesc layout is part of the C ABI (include/surya_amd.h, preprocess_gpu.py)");

constexpr int RECTIFY_TILE = 16;      // 16 x 16 output pixels per workgroup
constexpr int RECTIFY_BATCH = 32;     // descriptors per launch: 32 * 104 B + the header stay below the 4 KB of kernel arguments

struct RectifyArgs {
    const unsigned char* pages;
    unsigned char* out;          // may lie in the pages' allocation (disjoint range): no restrict anywhere
    int pix, n;
    RectifyDesc d[RECTIFY_BATCH];
};

// floor(s) as a tap base that is safe to turn into an int whatever s is (the host validates quads, the device only stays in bounds)
__device__ __forceinline__ long tap_base(double f, int len) {
    const double lo = -4.0, hi = (double)len + 4.0;
    return (long)(f < lo ? lo : (f > hi ? hi : f));
}

// The tap body of rectify_kernel and unroll_kernel (rec_unroll.h): the page is read at (sx, sy), pixel-index coordinates, and the
// rounded pixel written to dst. ONE function, so the two kernels cannot drift apart in a product or a sum.
__device__ __forceinline__ void warp_sample(const unsigned char* page, int page_w, int page_h, int pix, double sx, double sy,
                                            unsigned char* dst) {
#pragma clang fp contract(off)
    const double fx = floor(sx), fy = floor(sy);
    double wx[4], wy[4];
    cubic_w(sx - fx, wx);
    cubic_w(sy - fy, wy);
    const long bx = tap_base(fx, page_w), by = tap_base(fy, page_h);
    int xi[4], yi[4];
    for (int k = 0; k < 4; ++k) {
        const long x = bx - 1 + k, y = by - 1 + k;
        xi[k] = (int)(x < 0 ? 0 : (x > page_w - 1 ? page_w - 1 : x));         // replicate border
        yi[k] = (int)(y < 0 ? 0 : (y > page_h - 1 ? page_h - 1 : y));
    }
    double acc[3];
    for (int j = 0; j < 4; ++j) {
        const unsigned char* row = page + (long)yi[j] * page_w * pix;
        double h[3];
        for (int k = 0; k < 4; ++k) {
            double p[3];
            if (pix == 4) {                                   // page_off and the pixel offset are multiples of 4
                const uint32_t q = *reinterpret_cast<const uint32_t*>(row + (long)xi[k] * 4);
                p[0] = (double)(q & 0xff); p[1] = (double)((q >> 8) & 0xff); p[2] = (double)((q >> 16) & 0xff);
            } else {
                const unsigned char* px = row + (long)xi[k] * 3;
                p[0] = (double)px[0]; p[1] = (double)px[1]; p[2] = (double)px[2];
            }
            for (int c = 0; c < 3; ++c) h[c] = k == 0 ? p[c] * wx[0] : h[c] + p[c] * wx[k];
        }
        for (int c = 0; c < 3; ++c) acc[c] = j == 0 ? h[c] * wy[0] : acc[c] + h[c] * wy[j];
    }
    uint32_t b[3];
    for (int c = 0; c < 3; ++c) {
        const double r = rint(acc[c]);
        b[c] = (uint32_t)(int)(r < 0.0 ? 0.0 : (r > 255.0 ? 255.0 : r));
    }
    if (pix == 4) {
        *reinterpret_cast<uint32_t*>(dst) = b[0] | (b[1] << 8) | (b[2] << 16);
    } else {
        dst[0] = (unsigned char)b[0]; dst[1] = (unsigned char)b[1]; dst[2] = (unsigned char)b[2];
    }
}

__global__ __launch_bounds__(256) void rectify_kernel(RectifyArgs a) {
#pragma clang fp contract(off)
    const RectifyDesc& D = a.d[blockIdx.z];
    if ((int)blockIdx.x * RECTIFY_TILE >= D.out_w || (int)blockIdx.y * RECTIFY_TILE >= D.out_h) return;    // workgroup-uniform
    const int u = blockIdx.x * RECTIFY_TILE + (threadIdx.x & (RECTIFY_TILE - 1));
    const int v = blockIdx.y * RECTIFY_TILE + (threadIdx.x / RECTIFY_TILE);
    if (u >= D.out_w || v >= D.out_h) return;
    const double U = (double)u + 0.5, V = (double)v + 0.5;
    const double w = D.h[6] * U + D.h[7] * V + D.h[8];
    const double sx = (D.h[0] * U + D.h[1] * V + D.h[2]) / w - 0.5;
    const double sy = (D.h[3] * U + D.h[4] * V + D.h[5]) / w - 0.5;
    warp_sample(a.pages + D.page_off, D.page_w, D.page_h, a.pix, sx, sy, a.out + D.out_off + ((long)v * D.out_w + u) * a.pix);
}

// descs: HOST array of n descriptors, validated here (what the device then reads, it reads unchecked); nothing is launched unless
// every descriptor passes
static inline int rectify_run(const unsigned char* pages, const RectifyDesc* descs, int n, unsigned char* out, int pix, int max_w,
                              int max_h, hipStream_t s) {
    if (n < 0 || (pix != 3 && pix != 4)) return SA_ERR_ARG;
    if (n == 0) return SA_OK;
    if (!pages || !descs || !out || max_w <= 0 || max_h <= 0) return SA_ERR_ARG;
    for (int i = 0; i < n; ++i) {
        const RectifyDesc& d = descs[i];
        if (d.page_w <= 0 || d.page_h <= 0 || d.out_w <= 0 || d.out_h <= 0 || d.out_w > max_w || d.out_h > max_h) return SA_ERR_ARG;
        if (d.page_off < 0 || d.out_off < 0) return SA_ERR_ARG;
        if (pix == 4 && ((d.page_off | d.out_off) & 3)) return SA_ERR_ARG;
    }
    if (pix == 4 && ((reinterpret_cast<uintptr_t>(pages) | reinterpret_cast<uintptr_t>(out)) & 3)) return SA_ERR_ARG;
    const int tw = cdiv(max_w, RECTIFY_TILE), th = cdiv(max_h, RECTIFY_TILE);
    if (th > 65535) return SA_ERR_ARG;                        // grid.y / grid.z limits
    for (int i0 = 0; i0 < n; i0 += RECTIFY_BATCH) {
        RectifyArgs a;
        a.pages = pages; a.out = out; a.pix = pix; a.n = n - i0 < RECTIFY_BATCH ? n - i0 : RECTIFY_BATCH;
        for (int i = 0; i < RECTIFY_BATCH; ++i) a.d[i] = descs[i0 + (i < a.n ? i : 0)];
        hipLaunchKernelGGL(rectify_kernel, dim3(tw, th, a.n), dim3(256), 0, s, a);
    }
    return (int)hipGetLastError();
}

}  // namespace prep
}  // namespace sa
