// Centre-line profile of a text component: the integer arithmetic, shared by the HIP kernels (det_centerline.h) and a plain-C++ build
// (tests/native/det_centerline_host.cpp). surya_amd/detection/centerline.py states the whole rule; this is its per-pixel half.
//
//   axis      0 (bins along x, perpendicular coordinate p = y) when x1 - x0 >= y1 - y0 of the inclusive bounding box, else 1 (bins along
//             y, p = x). A tie is a horizontal line.
//   bin       k = (t * knots) / extent by integer division, t = the pixel's coordinate along the axis minus the box origin, extent = the
//             box length along the axis. extent <= 8192 and knots <= 64 keep t * knots below 2^19.
//   per bin   cnt (uint32) pixels, sum (uint64) of p, lo / hi (int32) = min / max of p. An empty bin: 0, 0, 0x7fffffff, -1.
//             sum <= 8192 * 8192 * 8191 < 2^39 for one bin of the largest map.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SA_CL_HD __host__ __device__ __forceinline__
#else
#define SA_CL_HD inline
#endif

namespace sa {
namespace centerline {

constexpr int CL_MAX_DIM = 8192;          // height and width limit: extent <= 8192
constexpr int CL_MIN_KNOTS = 2;
constexpr int CL_MAX_KNOTS = 64;
constexpr int CL_EMPTY_LO = 0x7fffffff;
constexpr int CL_EMPTY_HI = -1;

// (64-bit differences and the extent test below: a box made of arbitrary words gives no overflow and no bin outside [0, knots))
SA_CL_HD int cl_axis(int x0, int x1, int y0, int y1) { return ((int64_t)x1 - x0 >= (int64_t)y1 - y0) ? 0 : 1; }

struct ClFrame { int axis, origin, extent; };

SA_CL_HD ClFrame cl_frame(int x0, int x1, int y0, int y1) {
    ClFrame f;
    f.axis = cl_axis(x0, x1, y0, y1);
    f.origin = f.axis == 0 ? x0 : y0;
    const int64_t e = (f.axis == 0 ? (int64_t)x1 - x0 : (int64_t)y1 - y0) + 1;
    f.extent = (e >= 1 && e <= CL_MAX_DIM) ? (int)e : 0;              // 0: no pixel falls into this frame
    return f;
}

// bin of coordinate `a` along the axis; -1 when the pixel lies outside the frame (cannot happen for a pixel of the component itself)
SA_CL_HD int cl_bin(const ClFrame& f, int a, int knots) {
    const int64_t t = (int64_t)a - f.origin;
    if (t < 0 || t >= f.extent) return -1;
    return (int)(((uint32_t)t * (uint32_t)knots) / (uint32_t)f.extent);
}

// sum of the integers a, a + 1, ..., a + n - 1 (n >= 1, a >= 0)
SA_CL_HD uint64_t cl_arith_sum(int a, int n) { return (uint64_t)n * (uint64_t)a + (uint64_t)n * (uint64_t)(n - 1) / 2; }

}  // namespace centerline
}  // namespace sa
