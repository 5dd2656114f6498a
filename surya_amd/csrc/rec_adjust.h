// Contrast adjustment of line crops ON THE DEVICE: a crop of a page (or a rectified crop, rec_rectify.h) -> its adjusted, padded copy,
// written behind the pages as a small synthetic "page" that the line pre-processing (rec_prep.h) reads like any other page through
// (page_off, page_w, x0 = y0 = 0, has_poly = 0) -- LineDesc and the four prep kernels do not change.
//
// The rule is Pillow's ImageOps.autocontrast(crop, cutoff, preserve_tone=True, mask), byte for byte (adjust_core.h holds its
// arithmetic): 256 bins of the luma over the crop (a polygon line: over the pixels its mask keeps, the mask being the one
// prep_mask_*_kernel rasterise, from the same device functions); cutoff percent of the counts removed from the low end, then from
// the high end of what is left; lo / hi the first / last bin left; the LUT int(i * 255.0 / (hi - lo) - lo * scale) in float64 without
// contraction, the identity when hi <= lo; the LUT applied to the three channels of every pixel of the padded crop (outside the
// polygon: 255 first, then the LUT). With 4-byte pixels X is written as 0.
//
// Three passes per batch of descriptors (kernel arguments, like rectify_kernel: wave-uniform descriptor reads from scalar registers):
//   adjust_hist_kernel   grid (chunks of ADJ_CHUNK pixels, lines): a per-workgroup histogram in LDS (integer LDS atomics), merged into the
//                        line's 256 global counters by at most one integer atomic per non-empty bin and workgroup. Lines range from
//                        1 pixel to 256 x 1024 and a second-pass call may hold a handful of them, so one workgroup per line would
//                        leave a 262 144-pixel crop to one CU; chunks keep every CU busy whatever the mix. Counts are integers: any
//                        order of the adds gives the same bits.
//   adjust_lut_kernel    one workgroup of 256 lanes per line, lane i owning bin i: two block scans (low cut over the exclusive prefix,
//                        high cut over the exclusive suffix of what is left), lo / hi by LDS integer min / max, lut[i].
//   adjust_apply_kernel  grid as the histogram's: the line's LUT in LDS, one thread per pixel (one 32-bit load and store with RGBX).
// Every early exit depends on blockIdx and the descriptor only (workgroup-uniform); nothing outside a line's output range, its mask,
// its 256 counters, its LUT and its (lo, hi) pair is written.
#pragma once
#include "adjust_core.h"
#include "common.h"
#include "rec_prep.h"

namespace sa {
namespace prep {

using adjust::AdjustDesc;

constexpr int ADJUST_BATCH = 32;            // descriptors per launch: 32 * 88 B + the header stay below the 4 KB of kernel arguments
constexpr int ADJ_PER_THREAD = 16;
constexpr int ADJ_CHUNK = 256 * ADJ_PER_THREAD;       // pixels per workgroup

struct AdjustArgs {
    const unsigned char* pages;
    unsigned char* out;          // may lie in the pages' allocation (disjoint ranges, validated): no restrict anywhere
    unsigned char* mask;         // arena: per polygon line [h][w] bytes, 1 = inside / on the boundary
    unsigned int* hist;          // [n][256], zero before the histogram pass
    unsigned char* lut;          // [n][256]
    int* lohi;                   // [n][2]
    int pix, n, first;           // `first`: index of d[0] in the call (rows of hist / lut / lohi)
    AdjustDesc d[ADJUST_BATCH];
};

__global__ __launch_bounds__(256) void adjust_mask_rows_kernel(AdjustArgs a) {
    const AdjustDesc& D = a.d[blockIdx.y];
    if (!D.has_poly) return;
    poly_mask_rows(D.poly, D.w, D.h, a.mask + D.mask_off, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}

__global__ __launch_bounds__(256) void adjust_mask_edges_kernel(AdjustArgs a) {
    const AdjustDesc& D = a.d[blockIdx.y];
    if (!D.has_poly) return;
    poly_mask_edges(D.poly, D.w, D.h, a.mask + D.mask_off, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}

// the three channels of pixel i of a line's crop (i < w * h)
__device__ __forceinline__ void adjust_px(const AdjustArgs& a, const AdjustDesc& D, unsigned i, unsigned (&v)[3]) {
    const unsigned y = i / (unsigned)D.w, x = i - y * (unsigned)D.w;
    const unsigned char* px = a.pages + D.src_off + ((long)(D.y0 + (int)y) * D.src_w + (D.x0 + (int)x)) * a.pix;
    if (a.pix == 4) {                                       // src_off and the pixel offset are multiples of 4
        const uint32_t q = *reinterpret_cast<const uint32_t*>(px);
        v[0] = q & 0xff; v[1] = (q >> 8) & 0xff; v[2] = (q >> 16) & 0xff;
    } else {
        v[0] = px[0]; v[1] = px[1]; v[2] = px[2];
    }
}

__global__ __launch_bounds__(256) void adjust_hist_kernel(AdjustArgs a) {
    __shared__ unsigned int h[256];
    const AdjustDesc& D = a.d[blockIdx.y];
    const unsigned npx = (unsigned)D.w * (unsigned)D.h;
    const unsigned base = blockIdx.x * (unsigned)ADJ_CHUNK;
    if (base >= npx) return;                                  // workgroup-uniform
    const int tid = threadIdx.x;
    h[tid] = 0;
    __syncthreads();
    const unsigned char* m = a.mask + D.mask_off;
    for (int k = 0; k < ADJ_PER_THREAD; ++k) {
        const unsigned i = base + k * 256 + tid;
        if (i < npx && (!D.has_poly || m[i])) {
            unsigned v[3];
            adjust_px(a, D, i, v);
            atomicAdd(&h[adjust::luma(v[0], v[1], v[2])], 1u);
        }
    }
    __syncthreads();
    if (h[tid]) atomicAdd(&a.hist[(long)(a.first + blockIdx.y) * 256 + tid], h[tid]);
}

// inclusive scan of s[0..255] by 256 threads (every thread of the block calls it)
__device__ __forceinline__ void adjust_scan256(unsigned int* s, int tid) {
    for (int off = 1; off < 256; off <<= 1) {
        const unsigned int v = tid >= off ? s[tid - off] : 0u;
        __syncthreads();
        s[tid] += v;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void adjust_lut_kernel(AdjustArgs a) {
    __shared__ unsigned int s[256];
    __shared__ int lo_s, hi_s;
    const AdjustDesc& D = a.d[blockIdx.x];
    const long line = a.first + blockIdx.x;
    const int tid = threadIdx.x;
    const unsigned int h = a.hist[line * 256 + tid];
    if (tid == 0) { lo_s = 255; hi_s = 0; }                   // what Pillow's two searches leave on an empty histogram
    s[tid] = h;
    __syncthreads();
    adjust_scan256(s, tid);
    const unsigned int cut = adjust::cut_count(s[255], D.cutoff);
    const unsigned int r = adjust::bin_left(h, cut, s[tid] - h);              // low end: `before` = the exclusive prefix
    __syncthreads();
    s[255 - tid] = r;
    __syncthreads();
    adjust_scan256(s, tid);
    const unsigned int left = adjust::bin_left(r, cut, s[255 - tid] - r);     // high end: the exclusive suffix of what is left
    if (left) { atomicMin(&lo_s, tid); atomicMax(&hi_s, tid); }
    __syncthreads();
    const int lo = lo_s, hi = hi_s;
    a.lut[line * 256 + tid] = (unsigned char)adjust::lut_entry(tid, lo, hi);
    if (tid < 2) a.lohi[line * 2 + tid] = tid ? hi : lo;
}

__global__ __launch_bounds__(256) void adjust_apply_kernel(AdjustArgs a) {
    __shared__ unsigned char lut[256];
    const AdjustDesc& D = a.d[blockIdx.y];
    const unsigned npx = (unsigned)D.w * (unsigned)D.h;
    const unsigned base = blockIdx.x * (unsigned)ADJ_CHUNK;
    if (base >= npx) return;                                  // workgroup-uniform
    const int tid = threadIdx.x;
    lut[tid] = a.lut[(long)(a.first + blockIdx.y) * 256 + tid];
    __syncthreads();
    const unsigned char* m = a.mask + D.mask_off;
    unsigned char* dst0 = a.out + D.out_off;
    for (int k = 0; k < ADJ_PER_THREAD; ++k) {
        const unsigned i = base + k * 256 + tid;
        if (i >= npx) break;
        unsigned v[3] = {255u, 255u, 255u};                   // the pad outside the polygon, which goes through the LUT as well
        if (!D.has_poly || m[i]) adjust_px(a, D, i, v);
        const uint32_t b0 = lut[v[0]], b1 = lut[v[1]], b2 = lut[v[2]];
        unsigned char* dst = dst0 + (long)i * a.pix;
        if (a.pix == 4) {
            *reinterpret_cast<uint32_t*>(dst) = b0 | (b1 << 8) | (b2 << 16);
        } else {
            dst[0] = (unsigned char)b0; dst[1] = (unsigned char)b1; dst[2] = (unsigned char)b2;
        }
    }
}

// descs: HOST array of n descriptors, validated here (adjust::validate; what the device then reads, it reads unchecked); nothing is
// launched, cleared or written unless every descriptor passes. work: n * 1280 bytes (the counters, then the LUTs).
static inline int adjust_run(const unsigned char* pages, const AdjustDesc* descs, int n, unsigned char* out, unsigned char* mask,
                             void* work, int* lohi, int pix, hipStream_t s) {
    if (adjust::validate(descs, n, reinterpret_cast<uintptr_t>(pages), reinterpret_cast<uintptr_t>(out), mask != nullptr, pix)) return SA_ERR_ARG;
    if (n == 0) return SA_OK;
    if (!work || !lohi || (reinterpret_cast<uintptr_t>(work) & 3)) return SA_ERR_ARG;
    unsigned int* hist = static_cast<unsigned int*>(work);
    unsigned char* lut = static_cast<unsigned char*>(work) + (size_t)n * 1024;
    hipError_t e = hipMemsetAsync(hist, 0, (size_t)n * 1024, s);
    if (e != hipSuccess) return (int)e;
    for (int i0 = 0; i0 < n; i0 += ADJUST_BATCH) {
        AdjustArgs a;
        a.pages = pages; a.out = out; a.mask = mask; a.hist = hist; a.lut = lut; a.lohi = lohi; a.pix = pix; a.first = i0;
        a.n = n - i0 < ADJUST_BATCH ? n - i0 : ADJUST_BATCH;
        long max_px = 1;
        bool any_poly = false;
        for (int i = 0; i < ADJUST_BATCH; ++i) {
            a.d[i] = descs[i0 + (i < a.n ? i : 0)];
            if (i < a.n) {
                const long px = (long)a.d[i].w * a.d[i].h;
                max_px = px > max_px ? px : max_px;
                any_poly = any_poly || a.d[i].has_poly;
            }
        }
        const int chunks = (int)cdivl(max_px, ADJ_CHUNK);     // <= 2^28 / 4096
        if (any_poly) launch_poly_masks(adjust_mask_rows_kernel, adjust_mask_edges_kernel, a, a.n, s);
        hipLaunchKernelGGL(adjust_hist_kernel, dim3(chunks, a.n), dim3(256), 0, s, a);
        hipLaunchKernelGGL(adjust_lut_kernel, dim3(a.n), dim3(256), 0, s, a);
        hipLaunchKernelGGL(adjust_apply_kernel, dim3(chunks, a.n), dim3(256), 0, s, a);
    }
    return (int)hipGetLastError();
}

}  // namespace prep
}  // namespace sa
