// Unrolling of BENT text lines ON THE DEVICE: the band around a line's centre line -> an upright uint8 crop, written behind the pages as
// a small synthetic "page" that the line pre-processing (rec_prep.h) reads like any other, exactly as rec_rectify.h's crops are.
//
// The rule is warp_columns of surya_amd/common/imageops.py, restated per pixel: output column u has a centre C(u) on the centre line and a
// unit normal N(u) (curve_table makes both on the host, float64, arc-length parametrised); output pixel (u, v) samples its page at
// C(u) + (v + 0.5 - out_h / 2) N(u) - 0.5 per axis, and from there on it is warp_quad's words exactly -- the tap body is rec_rectify.h's
// warp_sample, the ONE function both kernels call.
//
// One thread per output pixel, 16 x 16 pixel workgroups (a bent band's footprint stays a compact patch of the page), no LDS. A column's
// four doubles are two 16-byte loads at consecutive addresses along u: the 16 lanes of a tile row read 512 contiguous bytes. Descriptors
// travel in the kernel-argument segment, UNROLL_BATCH lines per launch; the tables stay in device memory.
#pragma once
#include "common.h"
#include "rec_rectify.h"

namespace sa {
namespace prep {

struct UnrollDesc {
    long page_off;               // byte offset of the source page's first pixel in `pages`
    int page_w, page_h;
    int out_w, out_h;            // size of the unrolled crop (curve_table)
    long out_off;                // byte offset of the crop's first pixel in `out`
    long table_off;              // doubles into `tables`: the crop's [out_w][4] = (Cx, Cy, Nx, Ny) per column
};

static_assert(sizeof(UnrollDesc) == 40, "UnrollDesc layout is part of the C ABI (include/surya_amd.h, preprocess_gpu.py)");

constexpr int UNROLL_BATCH = 32;      // descriptors per launch

struct UnrollArgs {
    const unsigned char* pages;
    unsigned char* out;          // may lie in the pages' allocation (disjoint range): no restrict anywhere
    const double* tables;
    int pix, n;
    UnrollDesc d[UNROLL_BATCH];
};

typedef double f64x2 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(256) void unroll_kernel(UnrollArgs a) {
#pragma clang fp contract(off)
    const UnrollDesc& D = a.d[blockIdx.z];
    if ((int)blockIdx.x * RECTIFY_TILE >= D.out_w || (int)blockIdx.y * RECTIFY_TILE >= D.out_h) return;    // workgroup-uniform
    const int u = blockIdx.x * RECTIFY_TILE + (threadIdx.x & (RECTIFY_TILE - 1));
    const int v = blockIdx.y * RECTIFY_TILE + (threadIdx.x / RECTIFY_TILE);
    if (u >= D.out_w || v >= D.out_h) return;
    const f64x2* col = reinterpret_cast<const f64x2*>(a.tables + D.table_off + (long)u * 4);              // table_off is even: 16-byte aligned
    const f64x2 c = col[0], nrm = col[1];
    const double d = ((double)v + 0.5) - (double)D.out_h / 2.0;
    const double sx = c.x + d * nrm.x - 0.5;
    const double sy = c.y + d * nrm.y - 0.5;
    warp_sample(a.pages + D.page_off, D.page_w, D.page_h, a.pix, sx, sy, a.out + D.out_off + ((long)v * D.out_w + u) * a.pix);
}

// descs: HOST array of n descriptors, validated here (what the device then reads, it reads unchecked); nothing is launched unless
// every descriptor passes
static inline int unroll_run(const unsigned char* pages, const UnrollDesc* descs, int n, const double* tables, unsigned char* out, int pix,
                             int max_w, int max_h, hipStream_t s) {
    if (n < 0 || (pix != 3 && pix != 4)) return SA_ERR_ARG;
    if (n == 0) return SA_OK;
    if (!pages || !descs || !tables || !out || max_w <= 0 || max_h <= 0) return SA_ERR_ARG;
    for (int i = 0; i < n; ++i) {
        const UnrollDesc& d = descs[i];
        if (d.page_w <= 0 || d.page_h <= 0 || d.out_w <= 0 || d.out_h <= 0 || d.out_w > max_w || d.out_h > max_h) return SA_ERR_ARG;
        if (d.page_off < 0 || d.out_off < 0 || d.table_off < 0 || (d.table_off & 1)) return SA_ERR_ARG;
        if (pix == 4 && ((d.page_off | d.out_off) & 3)) return SA_ERR_ARG;
    }
    if (pix == 4 && ((reinterpret_cast<uintptr_t>(pages) | reinterpret_cast<uintptr_t>(out)) & 3)) return SA_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(tables) & 15) return SA_ERR_ARG;
    const int tw = cdiv(max_w, RECTIFY_TILE), th = cdiv(max_h, RECTIFY_TILE);
    if (th > 65535) return SA_ERR_ARG;                        // grid.y / grid.z limits
    for (int i0 = 0; i0 < n; i0 += UNROLL_BATCH) {
        UnrollArgs a;
        a.pages = pages; a.out = out; a.tables = tables; a.pix = pix; a.n = n - i0 < UNROLL_BATCH ? n - i0 : UNROLL_BATCH;
        for (int i = 0; i < UNROLL_BATCH; ++i) a.d[i] = descs[i0 + (i < a.n ? i : 0)];
        hipLaunchKernelGGL(unroll_kernel, dim3(tw, th, a.n), dim3(256), 0, s, a);
    }
    return (int)hipGetLastError();
}

}  // namespace prep
}  // namespace sa
