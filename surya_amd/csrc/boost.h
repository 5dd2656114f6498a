// Boosted decoding (surya_rec_set_boost; recognition/boost.py compiles the tables): the words of a user list are preferred, nothing is
// forbidden. A slot follows a sparse automaton as a lexicon slot does (lexicon.h: CSR tables, the slot's own mask-table row rewritten behind
// each token), but its row is the PREFERRED set S of the position, not an allowed set, and the automaton is total: a token without an edge
// takes the fallback transition -- to `out_state` (inside a word that follows no entry; no edges) for a word unit, to the slot's root for
// a boundary. The word-unit set is row `word_row` of the same mask table. Per step, while boosting is on:
//     lm_head, masked greedy epilogue   -> record A of every row, over S      (gemm.h / gemm_mx.h, unchanged)
//     lm_head, unmasked greedy epilogue -> record B, over every column        (a second partial buffer)
//     boost_head_kernel                 -> reduces both, boost_core.h decides: token, score, plain reading, box, fused next embedding
//     automaton_step_kernel<true>       -> the slot's next state and row   (lexicon.h: the lexicon's step kernel with the fallback)
// A slot that is not boosted (state -1) carries beta = +inf: record A alone, the bits of greedy_head2_kernel on it.
//
// The launch code below is the only place that launches the head and the boost's start and step: the engine (rec_engine.h) and the op
// hooks (surya_op_rec_boost_step / surya_op_rec_boost_head) both go through it. The kernels read the tables unchecked: the engine
// validates them on the host (automaton_core.h), a caller of the op hooks answers for its own. Plain vector stores and vector atomics only.
#pragma once
#include "kernels.h"
#include "lexicon.h"
#include "boost_core.h"

namespace sa {

#define SA_BOOST_STEP_THREADS SA_LEXICON_STEP_THREADS      // the same kernel template, one wave

struct BoostArgs : TotalOps {           // slot_root, slot_beta, out_state, word_row (lexicon.h)
    LexiconArgs lx;                     // the CSR tables, the mask table and slot_state = the slots' boost states (state_flags: all 0;
                                        // eos / pad / nop are never preferred)
};

// The boosted head: greedy_head2_kernel (kernels.h) on two records per row. `h` carries what that kernel takes (its forced / pattern /
// alternatives members stay empty), h.part record A's per-tile partials, part_b record B's, same tiling. Both rows of partials (<= 4 per
// thread each) and the bbox operands are requested before anything is waited for; each record is reduced in greedy_head2_kernel's own
// order -- the same shuffle tree, the same serial sum over the waves -- so on a row with beta = +inf token, score and box have that
// kernel's bits on record A. Every thread evaluates boost_core.h (the fused embedding needs the token everywhere); thread 0 writes.
template <typename T>
struct BoostHeadArgs {
    HeadArgs<T> h;
    const float4* part_b = nullptr;     // [rows][tiles_n]
    const float* slot_beta = nullptr;   // [slots]
    int* plain_token = nullptr;         // by slot, as out_token
    float* plain_prob = nullptr;
};

template <typename T>
__global__ __launch_bounds__(SA_HEAD_THREADS) void boost_head_kernel(BoostHeadArgs<T> g) {
    constexpr int NT = SA_HEAD_THREADS, NW = NT / 64, NP = 4, V = Ty<T>::V16, NB = 32 / V;
    const HeadArgs<T>& a = g.h;
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles_n = a.tiles_n, H = a.H;
    __shared__ float smax[2][NW], ssum[2][NW], red[NW];
    __shared__ int sidx[2][NW];
    const float4* la = a.part + (long)r * tiles_n;
    const float4* lb = g.part_b + (long)r * tiles_n;
    float4 pv[2][NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int t = min(tid + k * NT, tiles_n - 1);
        pv[0][k] = la[t];
        pv[1][k] = lb[t];
    }
    uint4 hv[NB], wv[NB];
    const T* hr = a.hidden + (long)r * H;
    const T* wr = a.wb + (long)wave * H;
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        const int c = (u * 64 + lane) * V, cc = c < H ? c : 0;
        hv[u] = *reinterpret_cast<const uint4*>(hr + cc);
        wv[u] = *reinterpret_cast<const uint4*>(wr + cc);
    }
    const int slot = a.row_slot[r];
    const int klen = a.kv_len[slot];
    const float beta = g.slot_beta[slot];
    const float bias_o = Ty<T>::ld(a.bb + wave);

    float best[2];
    int bi[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        best[q] = -INFINITY;
        bi[q] = 0x7fffffff;
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int vi = __float_as_int(pv[q][k].y);
            if (tid + k * NT < tiles_n && (pv[q][k].x > best[q] || (pv[q][k].x == best[q] && vi < bi[q]))) { best[q] = pv[q][k].x; bi[q] = vi; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best[q], o, 64);
            const int oi = __shfl_xor(bi[q], o, 64);
            if (ob > best[q] || (ob == best[q] && oi < bi[q])) { best[q] = ob; bi[q] = oi; }
        }
        if (lane == 0) { smax[q][wave] = best[q]; sidx[q][wave] = bi[q]; }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        best[q] = smax[q][0]; bi[q] = sidx[q][0];
#pragma unroll
        for (int w = 1; w < NW; ++w)
            if (smax[q][w] > best[q] || (smax[q][w] == best[q] && sidx[q][w] < bi[q])) { best[q] = smax[q][w]; bi[q] = sidx[q][w]; }
        // (record A of an empty set is -inf everywhere: its sum is 0, and exp(-inf - (-inf)) must not appear)
        const float ref = best[q] == -INFINITY ? 0.f : best[q];
        float se = 0.f;
#pragma unroll
        for (int k = 0; k < NP; ++k)
            if (tid + k * NT < tiles_n) se += pv[q][k].z * expf(pv[q][k].x - ref);
        se = wave_sum(se);
        if (lane == 0) ssum[q][wave] = se;
    }
    // bbox dot product of this wave's output while the sums settle
    float d = 0.f;
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        float hf[V], wf[V];
        unpack16(hv[u], hf, (T*)nullptr);
        unpack16(wv[u], wf, (T*)nullptr);
        float du = 0.f;
#pragma unroll
        for (int i = 0; i < V; ++i) du += hf[i] * wf[i];
        d += ((u * 64 + lane) * V < H) ? du : 0.f;
    }
    d = wave_sum(d);
    __syncthreads();
    float tot[2] = {0.f, 0.f};
#pragma unroll
    for (int w = 0; w < NW; ++w) { tot[0] += ssum[0][w]; tot[1] += ssum[1][w]; }
    const boost::Out o = boost::combine(best[0], bi[0], tot[0], best[1], bi[1], tot[1], beta);
    const int tok = o.token;
    const bool done = (tok == a.eos_id) || (tok == a.pad_id);
    const int tok_next = done ? a.pad_id : tok;
    if (tid == 0) {
        a.out_token[slot] = tok;
        a.out_score[slot] = done ? 0.f : 1.0f / o.tot;
        a.next_token[slot] = tok_next;
        a.kv_len[slot] = klen + a.len_inc;
        if (a.table) a.row_len[r] = min(klen + a.len_inc, a.Tmax - 1);
        g.plain_token[slot] = o.plain_token;
        g.plain_prob[slot] = o.plain_prob;
    }
    if (lane == 0 && wave < 6) {
        const float lin = Ty<T>::rnd(d + bias_o);
        const float sg = Ty<T>::rnd(1.0f / (1.0f + expf(-lin)));
        a.out_bbox[slot * 6 + wave] = (int)(sg * a.bbox_size);
    }
    if (a.table)
        embed_norm_row<T, NT>(a.table + (long)tok_next * H, a.x + (long)r * H, a.wnorm, a.y + (long)r * H, H, a.eps, red, a.y8, a.sy, a.srows, r);
}

// automaton_start_kernel<true> / automaton_step_kernel<true> (lexicon.h) on the boost's operands.
inline int launch_boost_start(const BoostArgs& b, const int* slots, const int* roots, const float* betas, int n, hipStream_t s) {
    return launch_automaton_start<true>(b.lx, b, slots, roots, betas, n, s);
}
inline int launch_boost_step(const BoostArgs& b, const int* row_slot, const int* out_token, int rows, hipStream_t s) {
    return launch_automaton_step<true>(b.lx, b, row_slot, out_token, rows, s);
}
// Where greedy_head_kernel<T, true> would have to run instead of the partials head (launch_head, kernels.h): SA_ERR_STATE, fused or not.
template <typename T>
int launch_boost_head(const BoostHeadArgs<T>& g, bool mx, hipStream_t s) {
    const HeadArgs<T>& a = g.h;
    if (a.rows <= 0) return SA_OK;
    if (a.tiles_n <= 0 || !g.part_b || !g.slot_beta || !g.plain_token || !g.plain_prob || a.best_tot || a.fh.table || a.ph.tok_class) return SA_ERR_ARG;
    if (!head2_ok(a.H, mx) || a.tiles_n > 4 * SA_HEAD_THREADS) return SA_ERR_STATE;
    BoostHeadArgs<T> k = g;
    if (!a.table) k.h.y8 = k.h.sy = nullptr;
    hipLaunchKernelGGL((boost_head_kernel<T>), dim3(a.rows), dim3(SA_HEAD_THREADS), 0, s, k);
    return (int)hipGetLastError();
}

}  // namespace sa
