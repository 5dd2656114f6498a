// Page pre-processing of the layout family ON THE DEVICE: uint8 pages -> the encoder's pixel_values, replacing the host chain of
// LayoutImageProcessor (surya_amd/layout/predictor.py; SuryaEncoderImageProcessor, surya/common/donut/processor.py:24-126) for layout
// and table recognition:
//   crop           a slicer strip (layout/slicer.py ImageSlicer._strips) is a rectangle of its page: no crop is ever copied;
//   resize         straight to the model size with the cubic resample of common/imageops.resize (shared helpers, cv_resample.h):
//                  half-pixel centres, replicate border at the CROP's edge, float64 taps, horizontal pass before vertical, sums in
//                  tap order, no FMA contraction, one cast to fp32; an axis that keeps its length is passed through;
//   to uint8       rint (ties to even), clip to [0, 255] (cv2.resize returns uint8 for uint8 input);
//   rescale        x * (1 / 255) in fp64, cast to fp32;
//   normalise      (x - mean) / std in fp32 with correctly rounded division.
// The output is bit-identical to the host chain (tests/test_gpu_layout_prep.py). One thread per output pixel (3 channels): 16 source
// taps per channel, served from L1 / L2 (neighbouring output pixels share them); the three channel planes are written coalesced.
#pragma once
#include "common.h"
#include "cv_resample.h"

namespace sa {
namespace lprep {

struct PageDesc {
    long page_off;               // byte offset of the page's first pixel in `pages` (uint8 HWC, `pix` bytes per pixel)
    int page_w, page_h;
    int x0, y0, cw, ch;          // crop rectangle inside the page (cw, ch >= 1)
};

static_assert(sizeof(PageDesc) == 32, "PageDesc layout is part of the C ABI (include/surya_amd.h, layout/preprocess_gpu.py)");

// Descriptors travel in the kernel arguments (no device staging buffer, no handle): CHUNK of them per launch, 2 KB.
constexpr int CHUNK = 64;

struct Args {
    const unsigned char* pages;
    float* out;                  // [n][3][out_h][out_w]: image i of this launch at out + i * 3 * out_h * out_w
    int pix, out_h, out_w;
    float mean[3], std[3];
    PageDesc d[CHUNK];
};

__global__ __launch_bounds__(256) void layout_prep_kernel(Args p) {
#pragma clang fp contract(off)
    const PageDesc& D = p.d[blockIdx.y];
    const int W = p.out_w, npx = p.out_h * p.out_w;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npx) return;
    const int oy = i / W, ox = i % W;
    const unsigned char* page = p.pages + D.page_off;
    const int pw = D.page_w, pix = p.pix, x0 = D.x0, y0 = D.y0;
    float v[3];
    prep::resample_px<4>([&](int y, int x, int c) { return (float)page[((long)(y0 + y) * pw + (x0 + x)) * pix + c]; },
                         D.ch, D.cw, p.out_h, W, oy, ox, v);
    float* dst = p.out + (long)blockIdx.y * 3 * npx + i;
    for (int c = 0; c < 3; ++c) {
        float q = rintf(v[c]);
        q = q > 0.f ? q : 0.f;                                   // np.clip's max / min: a rounded -0.0 becomes +0.0 there as well
        q = q < 255.f ? q : 255.f;
        const float r = (float)((double)q * (1.0 / 255.0));      // x * (1 / 255) in fp64, cast
        dst[(long)c * npx] = (r - p.mean[c]) / p.std[c];
    }
}

// Validates every descriptor on the host (a crop outside its page or a page beyond `pages_bytes` never reaches the device), then
// launches CHUNK images at a time. Enqueue only.
static inline int run(const unsigned char* pages, size_t pages_bytes, const PageDesc* descs, int n, int pix, const float* mean,
                      const float* std, int out_h, int out_w, float* out, hipStream_t s) {
    if (!pages || !descs || !mean || !std || !out || n < 0) return SA_ERR_ARG;
    if (pix != 3 && pix != 4) return SA_ERR_ARG;
    if (out_h <= 0 || out_w <= 0 || (long)out_h * out_w > (1L << 28)) return SA_ERR_SHAPE;
    for (int i = 0; i < n; ++i) {
        const PageDesc& D = descs[i];
        if (D.page_off < 0 || D.page_w <= 0 || D.page_h <= 0 || D.x0 < 0 || D.y0 < 0 || D.cw <= 0 || D.ch <= 0) return SA_ERR_SHAPE;
        if ((long)D.x0 + D.cw > D.page_w || (long)D.y0 + D.ch > D.page_h || (long)D.page_w * D.page_h > (1L << 40)) return SA_ERR_SHAPE;
        if ((unsigned long)D.page_off + (unsigned long)D.page_w * (unsigned long)D.page_h * (unsigned long)pix > pages_bytes) return SA_ERR_SHAPE;
    }
    if (n == 0) return SA_OK;
    const long plane = (long)out_h * out_w;
    Args a;
    a.pages = pages; a.pix = pix; a.out_h = out_h; a.out_w = out_w;
    for (int c = 0; c < 3; ++c) { a.mean[c] = mean[c]; a.std[c] = std[c]; }
    for (int i0 = 0; i0 < n; i0 += CHUNK) {
        const int m = n - i0 < CHUNK ? n - i0 : CHUNK;
        for (int k = 0; k < m; ++k) a.d[k] = descs[i0 + k];
        a.out = out + (long)i0 * 3 * plane;
        hipLaunchKernelGGL(layout_prep_kernel, dim3(cdiv((int)plane, 256), m), dim3(256), 0, s, a);
    }
    return (int)hipGetLastError();
}

}  // namespace lprep
}  // namespace sa
