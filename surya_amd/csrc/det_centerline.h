// Centre-line profiles of the kept text components ON THE DEVICE (surya_det_centerlines; the rule: surya_amd/detection/centerline.py, the
// arithmetic: det_centerline_core.h). Enqueued behind a surya_det_boxes call of the same (batch, height, width, max_boxes): it READS that
// call's workspace (post_layout: st, label, area, comp) and writes only its own five output arrays. Integers only, so the result does not
// depend on the order anything arrives in and numpy states it bit for bit.
//
//   1 init      every (page, component, bin) gets the empty bin (0, 0, 0x7fffffff, -1); axis[b][c] = the component's axis, or -1 beyond the
//               page's count and on a page that overflowed max_boxes.
//   2 sweep     one raster sweep over `label` with 16-byte loads: a lane holds 4 neighbouring pixels of one row, a wave 256 consecutive
//               pixels, a workgroup a span of CL_CHUNK = 4096. Pixel -> root (label) -> compact index (area[root]) -> box (comp) -> bin.
//               Text-like maps: the 4 pixels of a lane share (component, bin), and so do long stretches of lanes. Lanes whose four pixels
//               agree find the runs of equal (component, bin, row) with __shfl_up / __ballot; the FIRST lane of a run adds for the whole
//               run: its length, length * y (axis 0) or the arithmetic sum of its x (axis 1), and min / max. A lane whose pixels disagree
//               (a component's or a bin's border) merges its own four and adds what is left.
//               Noise-like maps, where one component holds half the page and every wave would land on its `knots` addresses: the
//               workgroup adopts ONE component (the first it meets), keeps that component's bins in LDS (integer LDS atomics, 64-bit
//               for the sums) and sends each occupied bin to memory once, when it ends. Everything else goes to memory directly.
//
// Whatever the workspace holds, nothing is read or written out of bounds: a label outside [0, H W), a compact index outside the page's
// count and a pixel outside its component's box are skipped.
#pragma once
#include "common.h"
#include "det_post.h"
#include "det_centerline_core.h"

#ifndef SA_DET_CL_LDS
#define SA_DET_CL_LDS 1                  // 0: no adopted component, every add goes to memory (for an A/B)
#endif
#ifndef SA_DET_CL_RUNS
#define SA_DET_CL_RUNS 1                 // 0: no runs across lanes, every lane adds for its own four pixels (for an A/B)
#endif

namespace sa {
namespace centerline {

constexpr int CL_THREADS = 256;
constexpr int CL_STEPS = 4;
constexpr int CL_CHUNK = CL_THREADS * 4 * CL_STEPS;       // pixels of a workgroup: 4096, one scan block of det_post.h

struct ClArgs {
    const post::PageState* st;       // [B]
    const int* label;                // [B][N] flattened: the root's raster index, -1 = background
    const int* area;                 // [B][N] at a root: its compact index, -1 = dropped
    const post::CompStats* comp;     // [B][max_boxes]
    int B, H, W, max_boxes, knots;
    uint32_t* cnt; unsigned long long* sum; int* lo; int* hi;      // [B][max_boxes][knots]
    int* axis;                       // [B][max_boxes]
};

__device__ __forceinline__ int cl_page_count(const ClArgs& p, int b) {
    if (p.st[b].overflow) return 0;
    const int n = p.st[b].n_sel;
    return n < 0 ? 0 : (n > p.max_boxes ? p.max_boxes : n);
}

__global__ __launch_bounds__(CL_THREADS) void centerline_init_kernel(ClArgs p) {
    const int b = blockIdx.y;
    const long j = (long)blockIdx.x * CL_THREADS + threadIdx.x;
    const long per_page = (long)p.max_boxes * p.knots;
    if (j >= per_page) return;
    const long o = (long)b * per_page + j;
    p.cnt[o] = 0u; p.sum[o] = 0ull; p.lo[o] = CL_EMPTY_LO; p.hi[o] = CL_EMPTY_HI;
    if (j < p.max_boxes) {
        int a = -1;
        if (j < cl_page_count(p, b)) {
            const post::CompStats c = p.comp[(long)b * p.max_boxes + j];
            a = cl_axis(c.x0, c.x1, c.y0, c.y1);
        }
        p.axis[(long)b * p.max_boxes + j] = a;
    }
}

struct ClBins {                      // the adopted component's bins, in LDS
    unsigned long long sum[CL_MAX_KNOTS];
    uint32_t cnt[CL_MAX_KNOTS];
    int lo[CL_MAX_KNOTS], hi[CL_MAX_KNOTS];
};

__device__ __forceinline__ void cl_emit(const ClArgs& p, long page_out, ClBins& bins, int chosen, int idx, int k, uint32_t n,
                                        unsigned long long s, int mn, int mx) {
    if (SA_DET_CL_LDS && idx == chosen) {
        atomicAdd(&bins.cnt[k], n); atomicAdd(&bins.sum[k], s); atomicMin(&bins.lo[k], mn); atomicMax(&bins.hi[k], mx);
    } else {
        const long o = page_out + (long)idx * p.knots + k;
        atomicAdd(&p.cnt[o], n); atomicAdd(&p.sum[o], s); atomicMin(&p.lo[o], mn); atomicMax(&p.hi[o], mx);
    }
}

__global__ __launch_bounds__(CL_THREADS) void centerline_sweep_kernel(ClArgs p) {
    __shared__ ClBins bins;
    __shared__ int s_chosen;
    const int b = blockIdx.y, t = threadIdx.x, lane = t & 63;
    const int n_sel = cl_page_count(p, b);
    if (n_sel == 0) return;                                                      // block-uniform: a blank or overflowed page
    const long N = (long)p.H * p.W;
    const int* lab = p.label + (long)b * N;
    const int* area = p.area + (long)b * N;
    const post::CompStats* comp = p.comp + (long)b * p.max_boxes;
    const long page_out = (long)b * p.max_boxes * p.knots;
    if (t < CL_MAX_KNOTS) { bins.sum[t] = 0ull; bins.cnt[t] = 0u; bins.lo[t] = CL_EMPTY_LO; bins.hi[t] = CL_EMPTY_HI; }
    if (t == 0) s_chosen = -1;
    for (int step = 0; step < CL_STEPS; ++step) {
        const long i = (long)blockIdx.x * CL_CHUNK + (long)(step * CL_THREADS + t) * 4;
        int idx[4] = {-1, -1, -1, -1}, bin[4] = {0, 0, 0, 0};
        int ax = 0, x = 0, y = 0;
        if (i < N) {                                                             // (N % 4 == 0: the four labels lie inside the page)
            const int4 v = *reinterpret_cast<const int4*>(lab + i);
            const int r4[4] = {v.x, v.y, v.z, v.w};
            y = (int)(i / p.W); x = (int)(i % p.W);                              // W % 4 == 0: the four pixels share a row
            int prev_r = -1, prev_idx = -1;
            ClFrame f{0, 0, 1};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = r4[e];
                if (r < 0 || (long)r >= N) { prev_r = -1; prev_idx = -1; continue; }
                if (r != prev_r) {
                    prev_r = r;
                    prev_idx = area[r];
                    if ((unsigned)prev_idx < (unsigned)n_sel) {
                        const post::CompStats c = comp[prev_idx];
                        f = cl_frame(c.x0, c.x1, c.y0, c.y1);
                    } else {
                        prev_idx = -1;
                    }
                }
                if (prev_idx < 0) continue;
                const int k = cl_bin(f, f.axis == 0 ? x + e : y, p.knots);
                if (k < 0) continue;
                idx[e] = prev_idx; bin[e] = k; ax = f.axis;                      // (ax is used only when the four agree)
            }
        }
        const bool any = idx[0] >= 0 || idx[1] >= 0 || idx[2] >= 0 || idx[3] >= 0;
        __syncthreads();                                                         // the bins are zeroed; the last step's adoption is visible
        if (SA_DET_CL_LDS && s_chosen < 0) {
            const unsigned long long anym = __ballot(any);
            if (anym && lane == __builtin_ctzll(anym)) {
                const int first = idx[0] >= 0 ? idx[0] : (idx[1] >= 0 ? idx[1] : (idx[2] >= 0 ? idx[2] : idx[3]));
                atomicCAS(&s_chosen, -1, first);
            }
        }
        __syncthreads();
        const int chosen = s_chosen;
        const bool whole = idx[0] >= 0 && idx[1] == idx[0] && idx[2] == idx[0] && idx[3] == idx[0] && bin[1] == bin[0] && bin[2] == bin[0] &&
                           bin[3] == bin[0];
#if SA_DET_CL_RUNS
        // runs of lanes whose four pixels agree on (component, bin) inside one row: the first lane adds for the run
        const int key = whole ? idx[0] * CL_MAX_KNOTS + bin[0] : -1;
        const int pkey = __shfl_up(key, 1), py = __shfl_up(y, 1);
        const bool head = lane == 0 || pkey != key || py != y;
        const unsigned long long heads = __ballot(head);
        if (whole && head) {
            const unsigned long long rest = (heads >> lane) >> 1;                // the heads behind this lane
            const int len = 4 * (rest ? __ffsll(rest) : 64 - lane);              // pixels up to the next head
            if (ax == 0) cl_emit(p, page_out, bins, chosen, idx[0], bin[0], (uint32_t)len, (unsigned long long)len * (unsigned long long)y, y, y);
            else cl_emit(p, page_out, bins, chosen, idx[0], bin[0], (uint32_t)len, cl_arith_sum(x, len), x, x + len - 1);
        }
        if (!whole && any) {
#else
        if (any) {
#endif
            // a border lane: merge equal neighbours among its own four pixels. The perpendicular coordinate follows from the pixel's own box.
            int e = 0;
            while (e < 4) {
                if (idx[e] < 0) { ++e; continue; }
                const post::CompStats c = comp[idx[e]];
                const int a = cl_axis(c.x0, c.x1, c.y0, c.y1);
                int q = e + 1;
                while (q < 4 && idx[q] == idx[e] && bin[q] == bin[e]) ++q;
                const int len = q - e;
                if (a == 0) cl_emit(p, page_out, bins, chosen, idx[e], bin[e], (uint32_t)len, (unsigned long long)len * (unsigned long long)y, y, y);
                else cl_emit(p, page_out, bins, chosen, idx[e], bin[e], (uint32_t)len, cl_arith_sum(x + e, len), x + e, x + q - 1);
                e = q;
            }
        }
    }
    __syncthreads();
    if (SA_DET_CL_LDS) {
        const int chosen = s_chosen;
        if (chosen >= 0 && t < p.knots && bins.cnt[t]) {
            const long o = page_out + (long)chosen * p.knots + t;
            atomicAdd(&p.cnt[o], bins.cnt[t]); atomicAdd(&p.sum[o], bins.sum[t]); atomicMin(&p.lo[o], bins.lo[t]); atomicMax(&p.hi[o], bins.hi[t]);
        }
    }
}

static inline int centerlines_run(int B, int H, int W, int max_boxes, int knots, const void* boxes_workspace, size_t workspace_bytes,
                                  uint32_t* cnt, uint64_t* sum, int32_t* lo, int32_t* hi, int32_t* axis, hipStream_t s) {
    if (!boxes_workspace || !cnt || !sum || !lo || !hi || !axis) return SA_ERR_ARG;
    if (B < 0 || H <= 0 || W <= 0 || max_boxes <= 0 || knots < CL_MIN_KNOTS || knots > CL_MAX_KNOTS) return SA_ERR_ARG;
    if (B > 65535 || (long)max_boxes * CL_MAX_KNOTS > 0x7fffffffL) return SA_ERR_ARG;            // grid.y; (component, bin) in one int
    if (W % 4 || H > CL_MAX_DIM || W > CL_MAX_DIM) return SA_ERR_SHAPE;                           // 16-byte row sweeps; extent <= 8192
    if (B == 0) return SA_OK;
    const post::PostLayout L = post::post_layout(B, H, W, max_boxes);
    if (workspace_bytes < L.total || ((uintptr_t)boxes_workspace % 16)) return SA_ERR_ARG;
    const char* w = reinterpret_cast<const char*>(boxes_workspace);
    ClArgs p;
    p.st = (const post::PageState*)(w + L.st); p.label = (const int*)(w + L.label); p.area = (const int*)(w + L.area);
    p.comp = (const post::CompStats*)(w + L.comp);
    p.B = B; p.H = H; p.W = W; p.max_boxes = max_boxes; p.knots = knots;
    p.cnt = cnt; p.sum = (unsigned long long*)sum; p.lo = lo; p.hi = hi; p.axis = axis;
    const long N = (long)H * W, per_page = (long)max_boxes * knots;
    hipLaunchKernelGGL(centerline_init_kernel, dim3((unsigned)cdivl(per_page, CL_THREADS), (unsigned)B), dim3(CL_THREADS), 0, s, p);
    hipLaunchKernelGGL(centerline_sweep_kernel, dim3((unsigned)cdivl(N, CL_CHUNK), (unsigned)B), dim3(CL_THREADS), 0, s, p);
    SA_HIP(hipGetLastError());
    return SA_OK;
}

}  // namespace centerline
}  // namespace sa
