// Per-pixel resampling of surya_amd/common/imageops.py (the restatement of cv2's INTER_CUBIC a = -0.75 / INTER_LANCZOS4 geometry used
// by the host paths), shared by the recognition line pre-processing (rec_prep.h) and the layout-family page pre-processing
// (layout_prep.h): half-pixel centres, replicate border, taps and sums in float64 with the same association (no FMA contraction),
// horizontal pass before vertical, result rounded to float32 once.
#pragma once
#include "common.h"

namespace sa {
namespace prep {

__device__ __forceinline__ void cubic_w(double t, double* w) {            // imageops._cubic_weights, a = -0.75
#pragma clang fp contract(off)
    const double a = -0.75;
    w[0] = ((a * (t + 1) - 5 * a) * (t + 1) + 8 * a) * (t + 1) - 4 * a;
    w[1] = ((a + 2) * t - (a + 3)) * t * t + 1;
    w[2] = ((a + 2) * (1 - t) - (a + 3)) * (1 - t) * (1 - t) + 1;
    w[3] = 1.0 - w[0] - w[1] - w[2];
}
__device__ __forceinline__ double sinc_pi(double x) {                     // np.sinc
    if (x == 0.0) return 1.0;
    const double y = 3.141592653589793238462643383279502884 * x;
    return sin(y) / y;
}
__device__ __forceinline__ void lanczos4_w(double t, double* w) {         // imageops._lanczos4_weights
#pragma clang fp contract(off)
    double s = 0.0;
    for (int i = 0; i < 8; ++i) {
        const double x = t - (double)(i - 3);
        double v = fabs(x) < 1e-12 ? 1.0 : sinc_pi(x) * sinc_pi(x / 4.0);
        if (fabs(x) >= 4.0) v = 0.0;
        w[i] = v;
    }
    // np.sum over 8 contiguous doubles: pairwise is not used below 8 elements' unrolled block -> numpy adds them with its
    // 8-accumulator loop only for n >= 8: r[0..7] each one element, combined as ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7))
    s = ((w[0] + w[1]) + (w[2] + w[3])) + ((w[4] + w[5]) + (w[6] + w[7]));
    for (int i = 0; i < 8; ++i) w[i] = w[i] / s;
}

template <int TAPS>
__device__ __forceinline__ void axis_setup(int out_i, int in_len, int out_len, int* idx, double* w) {
#pragma clang fp contract(off)
    const double scale = (double)in_len / (double)out_len;
    const double src = ((double)out_i + 0.5) * scale - 0.5;
    const double base = floor(src), t = src - base;
    if (TAPS == 4) cubic_w(t, w); else lanczos4_w(t, w);
    const int first = TAPS == 4 ? -1 : -3;
    for (int k = 0; k < TAPS; ++k) {
        long j = (long)base + first + k;
        idx[k] = (int)(j < 0 ? 0 : (j > in_len - 1 ? in_len - 1 : j));   // replicate border
    }
}

// out(y, x, :) of resampling a [in_h][in_w][3] source to [out_h][out_w]: horizontal pass first (per tap row), then vertical,
// float64 products and sequential sums like (gathered * w).sum(1) in imageops._resample_axis; an axis that keeps its length
// is passed through untouched (no taps), as there.
template <int TAPS, typename SRC>
__device__ __forceinline__ void resample_px(SRC src, int in_h, int in_w, int out_h, int out_w, int oy, int ox, float* out3) {
#pragma clang fp contract(off)
    int xi[TAPS], yi[TAPS];
    double wx[TAPS], wy[TAPS];
    const bool rx = in_w != out_w, ry = in_h != out_h;
    if (rx) axis_setup<TAPS>(ox, in_w, out_w, xi, wx);
    if (ry) axis_setup<TAPS>(oy, in_h, out_h, yi, wy);
    for (int c = 0; c < 3; ++c) {
        double acc = 0.0;
        const int ny = ry ? TAPS : 1;
        for (int j = 0; j < ny; ++j) {
            const int sy = ry ? yi[j] : oy;
            double h;
            if (rx) {
                h = (double)src(sy, xi[0], c) * wx[0];
                for (int k = 1; k < TAPS; ++k) h = h + (double)src(sy, xi[k], c) * wx[k];
            } else {
                h = (double)src(sy, ox, c);
            }
            if (ry) acc = j == 0 ? h * wy[0] : acc + h * wy[j];
            else acc = h;
        }
        out3[c] = (float)acc;
    }
}

}  // namespace prep
}  // namespace sa
