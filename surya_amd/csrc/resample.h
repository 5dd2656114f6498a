// Pillow's 8-bit LANCZOS resampler on the device (detection pages: Image.thumbnail + Image.resize of
// surya/detection/__init__.py:50-57; algorithm = Pillow src/libImaging/Resample.c, restated in surya_amd/common/pil_resample.py,
// which also builds the fixed-point coefficient tables on the host with the same libm). Byte / integer work, HBM-bound:
//   pass(out position o) = clip8((2^21 + sum_{t < n(o)} src[first(o) + t] * k[o][t]) >> 22), horizontal pass first into a uint8
//   intermediate, then the vertical pass over it -- bit-identical to Pillow by construction (int32 accumulation, arithmetic
//   shift, same tables).
// One thread per output pixel (3 channels); a row of output pixels reads a contiguous span of the source row.
// A source box (the fractional right / bottom edge thumbnail() passes after a reduce()) lives in the tables alone.
//
// Image.reduce((fx, fy)) (Pillow src/libImaging/Reduce.c; thumbnail's pre-pass for >= 4x shrinks): reduce_run below.
//   out[oy][ox] = ((sum + n / 2) * (2^24 / n)) >> 24 in uint32 over the n = nx * ny source pixels present in the block (ragged last
//   column / row / corner have their own n); the four (n / 2, 2^24 / n) pairs come from the host. It streams the largest pages the
//   detector sees (16-29 MB per strip) once: fx in {2, 3, 4} -- what real pages produce -- goes through reduce_span_kernel (a lane
//   loads the aligned 16 / 8 / 4-byte vectors that hold a few outputs' source pixels of a row, adjacent lanes adjacent spans, whole
//   blocks only; RGBX and packed RGB, which is how Pillow hands over pages above its 16 MB block size), everything else -- other
//   factors, unaligned rows, the ragged edges the span kernel leaves -- through reduce_generic_kernel on a rectangle of outputs.
#pragma once
#include "common.h"

namespace sa {
namespace rs {

struct PassArgs {
    const unsigned char* src; int sw, sh, spix;      // source [sh][sw][spix]
    unsigned char* dst; int dw, dh, dpix;            // destination [dh][dw][dpix]
    const int* bounds;                               // [out][2] = first source index, tap count
    const int* kk; int ksize;                        // [out][ksize] 22-bit fixed point
};

__device__ __forceinline__ unsigned char clip8(int v) {
    v >>= 22;                                        // arithmetic shift, as Pillow's clip8 lookup index
    return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}
__device__ __forceinline__ void put_px(unsigned char* d, int dpix, int s0, int s1, int s2) {
    if (dpix == 4) *reinterpret_cast<uint32_t*>(d) = (uint32_t)clip8(s0) | ((uint32_t)clip8(s1) << 8) | ((uint32_t)clip8(s2) << 16);
    else { d[0] = clip8(s0); d[1] = clip8(s1); d[2] = clip8(s2); }
}

__global__ __launch_bounds__(256) void resample_h_kernel(PassArgs a) {        // dh == sh
    const int xx = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (xx >= a.dw) return;
    const int x0 = a.bounds[2 * xx], n = a.bounds[2 * xx + 1];
    const int* k = a.kk + (long)xx * a.ksize;
    const unsigned char* p = a.src + ((long)y * a.sw + x0) * a.spix;
    int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
    for (int t = 0; t < n; ++t, p += a.spix) {
        const int kv = k[t];
        s0 += (int)p[0] * kv; s1 += (int)p[1] * kv; s2 += (int)p[2] * kv;
    }
    put_px(a.dst + ((long)y * a.dw + xx) * a.dpix, a.dpix, s0, s1, s2);
}

__global__ __launch_bounds__(256) void resample_v_kernel(PassArgs a) {        // dw == sw
    const int x = blockIdx.x * blockDim.x + threadIdx.x, yy = blockIdx.y;
    if (x >= a.dw) return;
    const int y0 = a.bounds[2 * yy], n = a.bounds[2 * yy + 1];
    const int* k = a.kk + (long)yy * a.ksize;                                  // block-uniform: scalar loads
    const unsigned char* p = a.src + ((long)y0 * a.sw + x) * a.spix;
    const long stride = (long)a.sw * a.spix;
    int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
    for (int t = 0; t < n; ++t, p += stride) {
        const int kv = k[t];
        s0 += (int)p[0] * kv; s1 += (int)p[1] * kv; s2 += (int)p[2] * kv;
    }
    put_px(a.dst + ((long)yy * a.dw + x) * a.dpix, a.dpix, s0, s1, s2);
}

__global__ __launch_bounds__(256) void repack_kernel(const unsigned char* src, int spix, unsigned char* dst, int dpix, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned char* p = src + i * spix;
    unsigned char* d = dst + i * dpix;
    d[0] = p[0]; d[1] = p[1]; d[2] = p[2];
    if (dpix == 4) d[3] = 0;
}

// ---- Image.reduce ----
struct ReduceArgs {
    const unsigned char* src; int sw, sh, spix;      // source [sh][sw][spix]
    unsigned char* dst; int dw, dpix;                // destination [ceil(sh / fy)][dw = ceil(sw / fx)][dpix]
    int fx, fy;
    unsigned amend[4], mult[4];                      // [last column | 2 * last row]: n / 2 and 2^24 / n of that kind of block
    int ox0, oy0, ox1, oy1;                          // the rectangle of outputs this launch writes
};

__device__ __forceinline__ void put_mean(unsigned char* d, int dpix, unsigned s0, unsigned s1, unsigned s2, unsigned amend, unsigned mult) {
    const unsigned r = ((s0 + amend) * mult) >> 24, g = ((s1 + amend) * mult) >> 24, b = ((s2 + amend) * mult) >> 24;
    if (dpix == 4) *reinterpret_cast<uint32_t*>(d) = r | (g << 8) | (b << 16);
    else { d[0] = (unsigned char)r; d[1] = (unsigned char)g; d[2] = (unsigned char)b; }
}

// Any factors, any source stride: one thread per output pixel of the rectangle, row-major over it (adjacent lanes = adjacent
// outputs of a row), grid-stride. DW: the source is RGBX at a 4-byte-aligned address, one dword load per pixel.
template <bool DW>
__global__ __launch_bounds__(256) void reduce_generic_kernel(ReduceArgs a) {
    const int rw = a.ox1 - a.ox0;
    const long total = (long)rw * (a.oy1 - a.oy0);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int oy = a.oy0 + (int)(i / rw), ox = a.ox0 + (int)(i % rw);
        const int x0 = ox * a.fx, y0 = oy * a.fy;
        const int nx = min(a.fx, a.sw - x0), ny = min(a.fy, a.sh - y0);
        const int kind = (nx < a.fx ? 1 : 0) | (ny < a.fy ? 2 : 0);
        unsigned s0 = 0, s1 = 0, s2 = 0;
        for (int y = 0; y < ny; ++y) {
            const unsigned char* p = a.src + ((long)(y0 + y) * a.sw + x0) * a.spix;
            for (int x = 0; x < nx; ++x, p += a.spix) {
                if (DW) {
                    const uint32_t v = *reinterpret_cast<const uint32_t*>(p);
                    s0 += v & 255u; s1 += (v >> 8) & 255u; s2 += (v >> 16) & 255u;
                } else { s0 += p[0]; s1 += p[1]; s2 += p[2]; }
            }
        }
        put_mean(a.dst + ((long)oy * a.dw + ox) * a.dpix, a.dpix, s0, s1, s2, a.amend[kind], a.mult[kind]);
    }
}

// fx in {2, 3, 4}, whole blocks only: a lane owns P adjacent outputs of a row = P * FX source pixels = NV vectors V (uint4, uint2
// or a dword) per source row, at an address aligned to V (the caller checks base and row pitch). SPIX = 3 takes the packed RGB
// bytes apart by their place in the lane's span. Lanes of a wave read adjacent segments; rows are dealt over blockIdx.y with a
// stride, so the grid stays capped.
template <int FX, int P, int SPIX, typename V>
__global__ __launch_bounds__(256) void reduce_span_kernel(ReduceArgs a) {
    constexpr int SPAN = P * FX * SPIX, NV = SPAN / (int)sizeof(V);                 // bytes and vectors per lane and row
    static_assert(NV * (int)sizeof(V) == SPAN, "a lane's span is a whole number of vectors");
    const int g = blockIdx.x * blockDim.x + threadIdx.x;                            // group of P outputs
    if (g >= a.ox1 / P) return;
    const long pitch = (long)a.sw * SPIX;
    for (int oy = blockIdx.y; oy < a.oy1; oy += gridDim.y) {
        const unsigned char* p = a.src + (long)oy * a.fy * pitch + (long)g * SPAN;
        unsigned s[P][3] = {};
#pragma unroll 2                                                                    // the loads of two source rows in flight per lane (fy = 2: all)
        for (int y = 0; y < a.fy; ++y, p += pitch) {
            V v[NV];
#pragma unroll
            for (int j = 0; j < NV; ++j) v[j] = reinterpret_cast<const V*>(p)[j];
            const uint32_t* d = reinterpret_cast<const uint32_t*>(v);
#pragma unroll
            for (int j = 0; j < P * FX; ++j)                                        // source pixel j of the span -> output j / FX
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int i = j * SPIX + c;                                     // its byte (a constant after unrolling)
                    s[j / FX][c] += (d[i >> 2] >> (8 * (i & 3))) & 255u;
                }
        }
        unsigned char* o = a.dst + ((long)oy * a.dw + (long)g * P) * a.dpix;
#pragma unroll
        for (int k = 0; k < P; ++k) put_mean(o + k * a.dpix, a.dpix, s[k][0], s[k][1], s[k][2], a.amend[0], a.mult[0]);
    }
}

template <typename K>
static inline void reduce_launch_rect(K kernel, ReduceArgs a, int ox0, int oy0, int ox1, int oy1, hipStream_t s) {
    if (ox1 <= ox0 || oy1 <= oy0) return;
    a.ox0 = ox0; a.oy0 = oy0; a.ox1 = ox1; a.oy1 = oy1;
    const long blocks = cdivl((long)(ox1 - ox0) * (oy1 - oy0), 256);
    hipLaunchKernelGGL(kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, a);
}

template <int FX, int P, int SPIX, typename V>
static inline void reduce_launch_span(ReduceArgs a, int* ox_done, int* oy_done, hipStream_t s) {
    const int groups = a.sw / (FX * P), rows = a.sh / a.fy;                          // whole blocks, whole groups of them
    if (groups <= 0 || rows <= 0) return;
    a.ox0 = a.oy0 = 0; a.ox1 = groups * P; a.oy1 = rows;
    const int gx = cdiv(groups, 256), cap = 4096 / gx > 0 ? 4096 / gx : 1;
    hipLaunchKernelGGL((reduce_span_kernel<FX, P, SPIX, V>), dim3(gx, rows < cap ? rows : cap), dim3(256), 0, s, a);
    *ox_done = a.ox1; *oy_done = rows;
}

// One Image.reduce((fx, fy)) of the whole image. The caller has checked strides, factors and sizes.
static inline int reduce_run(const unsigned char* src, int sw, int sh, int spix, unsigned char* dst, int dpix, int fx, int fy, hipStream_t s) {
    ReduceArgs a{};
    a.src = src; a.sw = sw; a.sh = sh; a.spix = spix; a.dst = dst; a.dw = cdiv(sw, fx); a.dpix = dpix; a.fx = fx; a.fy = fy;
    const int dh = cdiv(sh, fy);
    const int nx[2] = {fx, sw % fx ? sw % fx : fx}, ny[2] = {fy, sh % fy ? sh % fy : fy};
    for (int k = 0; k < 4; ++k) {
        const unsigned n = (unsigned)(nx[k & 1] * ny[k >> 1]);
        a.amend[k] = n / 2; a.mult[k] = (1u << 24) / n;                              // (255 n + n / 2) * (2^24 / n) < 2^32
    }
    // the span kernel takes the rectangle [0, ox_done) x [0, oy_done) of whole blocks, the generic one the right strip and the bottom row
    int ox_done = 0, oy_done = 0;
    const uintptr_t ad = (uintptr_t)src;
    const long pitch = (long)sw * spix;
    const int al = (ad % 16 == 0 && pitch % 16 == 0) ? 16 : (ad % 8 == 0 && pitch % 8 == 0) ? 8 : (ad % 4 == 0 && pitch % 4 == 0) ? 4 : 1;
    if (spix == 4) {
        if (fx == 2) { if (al == 16) reduce_launch_span<2, 2, 4, uint4>(a, &ox_done, &oy_done, s); else if (al == 8) reduce_launch_span<2, 1, 4, uint2>(a, &ox_done, &oy_done, s); }
        if (fx == 3) { if (al == 16) reduce_launch_span<3, 4, 4, uint4>(a, &ox_done, &oy_done, s); else if (al == 8) reduce_launch_span<3, 2, 4, uint2>(a, &ox_done, &oy_done, s); }
        if (fx == 4) { if (al == 16) reduce_launch_span<4, 1, 4, uint4>(a, &ox_done, &oy_done, s); else if (al == 8) reduce_launch_span<4, 1, 4, uint2>(a, &ox_done, &oy_done, s); }
    } else if (al >= 4) {     // dwords: 16-byte loads of 8 outputs' RGB per lane measured slower (6000 x 1024 strips by (2, 2): 12.6 against 8.1 us per call)
        if (fx == 2) reduce_launch_span<2, 2, 3, uint32_t>(a, &ox_done, &oy_done, s);
        if (fx == 3) reduce_launch_span<3, 4, 3, uint32_t>(a, &ox_done, &oy_done, s);
        if (fx == 4) reduce_launch_span<4, 1, 3, uint32_t>(a, &ox_done, &oy_done, s);
    }
    if (spix == 4 && ad % 4 == 0) {
        reduce_launch_rect(reduce_generic_kernel<true>, a, ox_done, 0, a.dw, oy_done, s);
        reduce_launch_rect(reduce_generic_kernel<true>, a, 0, oy_done, a.dw, dh, s);
    } else {
        reduce_launch_rect(reduce_generic_kernel<false>, a, ox_done, 0, a.dw, oy_done, s);
        reduce_launch_rect(reduce_generic_kernel<false>, a, 0, oy_done, a.dw, dh, s);
    }
    return (int)hipGetLastError();
}

// One ImagingResample: horizontal pass (if the width changes) into `tmp` ([sh][dw][4]), vertical pass (if the height changes).
static inline int resample_run(const unsigned char* src, int sw, int sh, int spix, unsigned char* dst, int dw, int dh, int dpix,
                               const int* bx, const int* kx, int ksx, const int* by, const int* ky, int ksy, unsigned char* tmp,
                               hipStream_t s) {
    const bool need_h = dw != sw, need_v = dh != sh;
    if (!need_h && !need_v) {
        hipLaunchKernelGGL(repack_kernel, dim3((unsigned)cdivl((long)sw * sh, 256)), dim3(256), 0, s, src, spix, dst, dpix, (long)sw * sh);
        return (int)hipGetLastError();
    }
    const unsigned char* cur = src;
    int cw = sw, cpix = spix;
    if (need_h) {
        if (!bx || !kx || (need_v && !tmp)) return SA_ERR_ARG;
        PassArgs a{src, sw, sh, spix, need_v ? tmp : dst, dw, sh, need_v ? 4 : dpix, bx, kx, ksx};
        hipLaunchKernelGGL(resample_h_kernel, dim3(cdiv(dw, 256), sh), dim3(256), 0, s, a);
        cur = tmp; cw = dw; cpix = 4;
    }
    if (need_v) {
        if (!by || !ky) return SA_ERR_ARG;
        PassArgs a{cur, cw, sh, cpix, dst, dw, dh, dpix, by, ky, ksy};
        hipLaunchKernelGGL(resample_v_kernel, dim3(cdiv(dw, 256), dh), dim3(256), 0, s, a);
    }
    return (int)hipGetLastError();
}

}  // namespace rs
}  // namespace sa
