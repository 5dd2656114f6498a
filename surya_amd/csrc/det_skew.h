// Page skew from the heat map ON THE DEVICE (surya_det_skew; the rule: surya_amd/detection/skew.py, the arithmetic: det_skew_core.h).
// The projection profile of the text pixels under every candidate angle, scored by the sum of squared differences of neighbouring bins
// (Postl; leptonica's pixFindSkew). Integers only: bins from 16.16 fixed-point coefficients made on the host, counts by integer atomics,
// scores in uint64 -- the result does not depend on the order anything arrives in, so numpy states it bit for bit.
//
//   1 compact   one sweep over the maps (16-byte loads): every text pixel goes as (y << 16) | x into its page's list in the workspace.
//               A block counts its 4096 pixels, takes its place in the list with ONE returning atomic on the page's counter (n_text
//               itself) and writes. The order of the list is not deterministic and does not matter.
//   2 score     grid (angle, page), 256 threads: an (H + W)-word histogram in LDS, the page's list walked once with LDS integer atomics,
//               then the squared differences in 64-bit integers and one plain store. A wave looks at 64 consecutive list entries, which
//               near 0 degrees are 64 neighbours of one map row and so ONE bin: lanes with their left neighbour's bin stay out and the
//               first lane of every run adds the run's length (SA_DET_SKEW_COMBINE=0 builds the one-add-per-pixel form for an A/B).
//               All workgroups of a call fit the chip at once (121 x 16 of them on 256 CUs x 8), so the pass takes as long as ONE
//               workgroup's walk of its list, a chain of load -> add: a lane keeps SKEW_WALK = 4 entries in flight.
//               LDS: 4 (H + W) + 32 bytes: 8 KiB at 1024^2, where the 256-thread limit of 8 workgroups per CU binds; 64 KiB at
//               8192^2, where two workgroups share a CU's 160 KiB. A blank page's workgroups store 0 and leave before they touch LDS.
//
// Re-reading a map once per angle would be n_angles x 4 H W bytes per page; the list of a text page is a few hundred KB and stays in L2.
#pragma once
#include "common.h"
#include "det_skew_core.h"

#ifndef SA_DET_SKEW_COMBINE
#define SA_DET_SKEW_COMBINE 1
#endif
#ifndef SA_DET_SKEW_WALK
#define SA_DET_SKEW_WALK 4
#endif

namespace sa {
namespace skew {

constexpr int SKEW_THREADS = 256;
constexpr int SKEW_WALK = SA_DET_SKEW_WALK;      // list entries a lane of the score kernel has in flight (=1: one at a time, for an A/B)
constexpr int SKEW_CHUNK = 4096;          // pixels a block compacts per step (256 threads x 4 loads x 4 floats)

__global__ __launch_bounds__(SKEW_THREADS) void skew_compact_kernel(const float* __restrict__ heat, long page_stride, int H, int W,
                                                                   float threshold, uint32_t* __restrict__ list, int* __restrict__ n_text) {
    __shared__ int wtot[SKEW_THREADS / 64];
    __shared__ int s_base;
    const int b = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long N = (long)H * W;
    const float* src = heat + (long)b * page_stride;
    uint32_t* dst = list + (size_t)b * N;
    for (long c0 = (long)blockIdx.x * SKEW_CHUNK; c0 < N; c0 += (long)gridDim.x * SKEW_CHUNK) {
        unsigned int mask = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long i = c0 + (long)(j * SKEW_THREADS + t) * 4;
            if (i < N) {                                                          // (N % 4 == 0: the four floats lie inside the page)
                const f32x4 v = *reinterpret_cast<const f32x4*>(src + i);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (skew_is_text(v[e], threshold)) mask |= 1u << (j * 4 + e);
            }
        }
        const int cnt = __popc(mask);
        int inc = cnt;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(inc, d);
            if (lane >= d) inc += o;
        }
        if (lane == 63) wtot[wave] = inc;
        __syncthreads();
        if (t == 0) {
            int tot = 0;
#pragma unroll
            for (int w = 0; w < SKEW_THREADS / 64; ++w) tot += wtot[w];
            s_base = tot ? atomicAdd(&n_text[b], tot) : 0;
        }
        __syncthreads();
        long pos = (long)s_base + inc - cnt;
        for (int w = 0; w < wave; ++w) pos += wtot[w];
        if (mask) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long i = c0 + (long)(j * SKEW_THREADS + t) * 4;
                const int y = (int)(i / W), x = (int)(i % W);                     // W % 4 == 0: the four pixels share a row
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if ((mask >> (j * 4 + e)) & 1u) {
                        if (pos >= 0 && pos < N) dst[pos] = skew_pack(x + e, y);  // (a counter that was not 0 at the start writes nothing outside)
                        ++pos;
                    }
            }
        }
        __syncthreads();                                                          // wtot / s_base are rewritten by the next step
    }
}

__global__ __launch_bounds__(SKEW_THREADS) void skew_score_kernel(const uint32_t* __restrict__ list, const int* __restrict__ n_text,
                                                                 const int32_t* __restrict__ cs, int n_angles, int H, int W,
                                                                 unsigned long long* __restrict__ scores) {
    extern __shared__ uint32_t skew_lds[];                // nb bins (rounded up to an even count), then one uint64 per wave
    const int a = blockIdx.x, b = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int nb = H + W;
    const long N = (long)H * W;
    long n = n_text[b];
    n = n < 0 ? 0 : (n > N ? N : n);
    unsigned long long* out = scores + (size_t)b * n_angles + a;
    if (n == 0) {                                         // block-uniform
        if (t == 0) *out = 0ull;
        return;
    }
    uint32_t* hist = skew_lds;
    unsigned long long* part = reinterpret_cast<unsigned long long*>(skew_lds + ((nb + 1) & ~1));
    for (int r = t; r < nb; r += SKEW_THREADS) hist[r] = 0;
    const int c = cs[((size_t)b * n_angles + a) * 2], s = cs[((size_t)b * n_angles + a) * 2 + 1];      // block-uniform: scalar loads
    const int off = skew_offset(W, s);
    const uint32_t* src = list + (size_t)b * N;
    __syncthreads();
    for (long base = t - lane; base < n; base += SKEW_WALK * SKEW_THREADS) {      // wave-uniform trip count
        uint32_t p[SKEW_WALK];
#pragma unroll
        for (int k = 0; k < SKEW_WALK; ++k) {                                     // the loads of a step are issued before its first add
            const long i = base + (long)k * SKEW_THREADS + lane;
            p[k] = i < n ? src[i] : 0xffffffffu;
        }
#pragma unroll
        for (int k = 0; k < SKEW_WALK; ++k) {
            int r = -1;
            if (base + (long)k * SKEW_THREADS + lane < n) {
                r = skew_bin(skew_packed_x(p[k]), skew_packed_y(p[k]), c, s, off);
                if ((unsigned)r >= (unsigned)nb) r = -1;                          // a bin outside [0, nb) is not counted
            }
#if SA_DET_SKEW_COMBINE
            const int prev = __shfl_up(r, 1);
            const bool head = lane == 0 || prev != r;
            const unsigned long long heads = __ballot(head);
            if (head && r >= 0) {
                const unsigned long long rest = (heads >> lane) >> 1;             // the heads behind this lane
                atomicAdd(&hist[r], (uint32_t)(rest ? __ffsll(rest) : 64 - lane));    // run length = distance to the next head
            }
#else
            if (r >= 0) atomicAdd(&hist[r], 1u);
#endif
        }
    }
    __syncthreads();
    unsigned long long acc = 0;
    for (int r = t; r < nb - 1; r += SKEW_THREADS) acc += skew_sqdiff(hist[r + 1], hist[r]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_down(acc, d);
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    if (t == 0) {
        unsigned long long tot = 0;
#pragma unroll
        for (int w = 0; w < SKEW_THREADS / 64; ++w) tot += part[w];
        *out = tot;
    }
}

static inline size_t skew_workspace_bytes(int B, int H, int W) { return (size_t)B * H * W * sizeof(uint32_t); }

static inline size_t skew_lds_bytes(int H, int W) { return (size_t)((H + W + 1) & ~1) * 4 + (SKEW_THREADS / 64) * 8; }

static inline int skew_run(const float* heat, long page_stride, int B, int H, int W, float threshold, const int32_t* cs, int n_angles,
                           uint64_t* scores, int32_t* n_text, void* workspace, size_t workspace_bytes, hipStream_t s) {
    if (!heat || !cs || !scores || !n_text || !workspace || B < 0 || H <= 0 || W <= 0) return SA_ERR_ARG;
    if (n_angles < 1 || n_angles > SKEW_MAX_ANGLES || !(threshold >= 0.f)) return SA_ERR_ARG;      // (!(x >= 0) refuses NaN too)
    if (H > SKEW_MAX_DIM || W > SKEW_MAX_DIM || W % 4 || (page_stride % 4) || ((uintptr_t)heat % 16)) return SA_ERR_SHAPE;
    if (B > 65535) return SA_ERR_ARG;                                                            // grid.y
    if (workspace_bytes < skew_workspace_bytes(B, H, W) || ((uintptr_t)workspace % 4)) return SA_ERR_ARG;
    if (B == 0) return SA_OK;
    const long N = (long)H * W;
    SA_HIP(hipMemsetAsync(n_text, 0, (size_t)B * sizeof(int32_t), s));
    const dim3 sweep((unsigned)std::min<long>(1024, cdivl(N, SKEW_CHUNK)), (unsigned)B);
    hipLaunchKernelGGL(skew_compact_kernel, sweep, dim3(SKEW_THREADS), 0, s, heat, page_stride, H, W, threshold, (uint32_t*)workspace,
                       (int*)n_text);
    static AttrOnce attr;
    const size_t lds = skew_lds_bytes(H, W);
    attr.ensure(skew_score_kernel, lds);
    hipLaunchKernelGGL(skew_score_kernel, dim3((unsigned)n_angles, (unsigned)B), dim3(SKEW_THREADS), lds, s, (const uint32_t*)workspace,
                       (const int*)n_text, cs, n_angles, H, W, (unsigned long long*)scores);
    SA_HIP(hipGetLastError());
    return SA_OK;
}

}  // namespace skew
}  // namespace sa
