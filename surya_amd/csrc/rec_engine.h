// RecModel<T>: the recognition engine behind surya_rec_* (host-side planning + kernel sequencing), as a header so that each compute
// dtype is instantiated in a translation unit of its own: float and bf16_t in rec_model.hip, fp16_t in rec_model_f16.hip (a second
// 16-bit engine in one object would set the build's wall time). Everything here is a template, a plain struct or static. What does
// not depend on T -- the modes' state and setters, the blocks, the host checks -- is RecBase in rec_state.h.
#pragma once
#include <memory>

#include "rec_state.h"
#include "decode_attn.h"
#include "kv_fanout.h"
#include "kv_store.h"
#include "attn_mfma.h"
#include "beam.h"

namespace sa {

// ------------------------------------------------------------------------------------------- encoder plan
struct EncPlan {
    int P = 0;
    std::vector<int> src_row, pos_hw, merged_src, hidx, widx;
    std::vector<int> win_cu, img_cu;            // segment boundaries in patches
};

// Index math of get_window_index / rot_pos_emb / get_2d_learned_embeddings for images [0, n) of grid_hw.
static int plan_encoder(const surya_rec_config& c, const int32_t* grid_hw, int n, EncPlan& pl) {
    const int mg = c.merge, unit = mg * mg, vw = c.window_tokens;
    pl = EncPlan();
    pl.win_cu.push_back(0);
    pl.img_cu.push_back(0);
    int tok_base = 0;
    for (int im = 0; im < n; ++im) {
        const int h = grid_hw[2 * im], w = grid_hw[2 * im + 1];
        if (h <= 0 || w <= 0 || h % mg || w % mg) return SA_ERR_SHAPE;
        const int lh = h / mg, lw = w / mg;
        const int pad_h = vw - lh % vw, pad_w = vw - lw % vw;      // == vw when divisible: one empty window row
        const int nh = (lh + pad_h) / vw, nw = (lw + pad_w) / vw;
        for (int wy = 0; wy < nh; ++wy)
            for (int wx = 0; wx < nw; ++wx) {
                int cnt = 0;
                for (int dy = 0; dy < vw; ++dy)
                    for (int dx = 0; dx < vw; ++dx) {
                        const int y = wy * vw + dy, x = wx * vw + dx;
                        if (y >= lh || x >= lw) continue;
                        const int tok = y * lw + x;
                        pl.merged_src.push_back(tok_base + tok);
                        // get_2d_learned_embeddings: (arange(n) / max(1, n-1) * mult).long() in fp32
                        pl.hidx.push_back((int)(((float)y / (float)std::max(1, lh - 1)) * (float)c.embed_multiplier));
                        pl.widx.push_back((int)(((float)x / (float)std::max(1, lw - 1)) * (float)c.embed_multiplier));
                        for (int u = 0; u < unit; ++u) {
                            pl.src_row.push_back((tok_base + tok) * unit + u);
                            pl.pos_hw.push_back(y * mg + u / mg);
                            pl.pos_hw.push_back(x * mg + u % mg);
                        }
                        ++cnt;
                    }
                if (cnt) pl.win_cu.push_back(pl.win_cu.back() + cnt * unit);   // unique_consecutive drops empties
            }
        tok_base += lh * lw;
        pl.img_cu.push_back(pl.img_cu.back() + h * w);
    }
    pl.P = pl.img_cu.back();
    return SA_OK;
}

struct SegLists {   // host side of AttnSegs
    std::vector<int> tile_seg, tile_q0, seg_len;
    std::vector<long> q_off, k_off, v_off, o_off;
    void add_tiles(int seg, int L) {
        for (int q0 = 0; q0 < L; q0 += 64) { tile_seg.push_back(seg); tile_q0.push_back(q0); }
    }
};

static AttnSegs stage_segs(Stager& st, const SegLists& s) {
    AttnSegs a;
    a.tile_seg = st.put(s.tile_seg); a.tile_q0 = st.put(s.tile_q0); a.seg_len = st.put(s.seg_len);
    a.q_off = st.put(s.q_off); a.k_off = st.put(s.k_off); a.v_off = st.put(s.v_off); a.o_off = st.put(s.o_off);
    return a;
}

template <int I> using HeadEpi = std::integral_constant<int, I>;      // compile-time index into a weight format's lm_head epilogues (heads())

template <typename T>
struct RecModel : RecBase {
    T* emb_ahead = nullptr;                              // [max_prefill_tokens][dec_hidden] image embeddings encoded ahead
    // encoder workspaces
    T *tiles_t, *ex, *eh, *eqkv, *emlp, *emh, *emerged;
    // decoder workspaces
    T *dx, *dh, *dqkv, *dattn, *dmlp, *dlast;
    float* logits;
    float2* erope;           // [max_patches][enc head_dim / 2] (cos, sin) of the vision rotary embedding
    float4* amax;            // greedy-head partials of the lm_head GEMM: [slot row][column tile]
    float2* rope_cs;                                     // decoder RoPE table [max_kv_len][head_dim/2] (cos, sin)
    float* part;                                         // split-K partial sums [8][max_slots][max(qkv_dim, hidden)]
    T *kcache, *vcache;
    static constexpr bool MX_OK = std::is_same<T, bf16_t>::value;     // MXFP8 weights / activations exist beside the bf16 engine only
    const T* W(int idx) const { return reinterpret_cast<const T*>(w[idx]); }
    const T* WE(int l, int k) const { return W(SA_RW_ENC(l, k)); }
    const T* WD(int l, int k) const { return W(SA_RW_DEC(c.enc_depth, l, k)); }

    static size_t layout(const surya_rec_config& c, RecModel* m) {
        Carve cv;
        const size_t Pm = c.max_patches, Tm = std::max(c.max_prefill_tokens, c.max_slots), S = c.max_slots;
        const int unit = c.merge * c.merge;
        const size_t qkv_d = (size_t)(c.dec_heads + 2 * c.dec_kv_heads) * c.dec_head_dim;
        size_t o_tiles = cv.take(Pm * c.patch_dim_pad * sizeof(T));
        size_t o_ex = cv.take(Pm * c.enc_hidden * sizeof(T));
        size_t o_eh = cv.take(Pm * c.enc_hidden * sizeof(T));
        size_t o_eqkv = cv.take(Pm * 3 * c.enc_hidden * sizeof(T));
        size_t o_emlp = cv.take(Pm * c.enc_inter_pad * sizeof(T));
        size_t o_emh = cv.take(Pm * c.enc_hidden * sizeof(T));                 // [P/unit, unit*He]
        size_t o_erope = cv.take(Pm * (size_t)(c.enc_hidden / c.enc_heads / 2) * sizeof(float2));
        size_t o_emerged = cv.take(Pm / unit * c.enc_out_hidden * sizeof(T));
        size_t o_dx = cv.take(Tm * c.dec_hidden * sizeof(T));
        size_t o_dh = cv.take(Tm * c.dec_hidden * sizeof(T));
        size_t o_dqkv = cv.take(Tm * qkv_d * sizeof(T));
        size_t o_dattn = cv.take(Tm * c.dec_heads * c.dec_head_dim * sizeof(T));
        size_t o_dmlp = cv.take(Tm * c.dec_inter * sizeof(T));
        size_t o_dlast = cv.take(S * c.dec_hidden * sizeof(T));
        size_t o_ahead = cv.take(Tm * c.dec_hidden * sizeof(T));
        size_t o_logits = cv.take(S * (size_t)c.vocab * sizeof(float));
        size_t o_amax = cv.take(S * (size_t)cdiv(c.vocab, 32) * sizeof(float4));
        size_t o_rope = cv.take((size_t)c.max_kv_len * (c.dec_head_dim / 2) * sizeof(float2));
        size_t o_part = cv.take((size_t)8 * S * std::max(qkv_d, (size_t)c.dec_hidden) * sizeof(float));
        const size_t kv_elems = (size_t)c.dec_layers * S * c.dec_kv_heads * c.max_kv_len * c.dec_head_dim;
        size_t o_k = cv.take(kv_elems * sizeof(T));
        size_t o_v = cv.take(kv_elems * sizeof(T));
        size_t o_kvlen = cv.take(S * sizeof(int));
        size_t o_next = cv.take(S * sizeof(int));
        size_t o_active = cv.take(S * sizeof(int));
        size_t o_rowlen = cv.take(S * sizeof(int));
        size_t o_out = cv.take((size_t)SA_MAX_STEPS * S * 8 * sizeof(int));
        if (m) {
            char* b = m->blk[RecBase::B_MAIN].dev;
            m->tiles_t = (T*)(b + o_tiles); m->ex = (T*)(b + o_ex); m->eh = (T*)(b + o_eh); m->eqkv = (T*)(b + o_eqkv);
            m->emlp = (T*)(b + o_emlp); m->emh = (T*)(b + o_emh); m->emerged = (T*)(b + o_emerged); m->erope = (float2*)(b + o_erope);
            m->dx = (T*)(b + o_dx); m->dh = (T*)(b + o_dh); m->dqkv = (T*)(b + o_dqkv); m->dattn = (T*)(b + o_dattn);
            m->dmlp = (T*)(b + o_dmlp); m->dlast = (T*)(b + o_dlast); m->emb_ahead = (T*)(b + o_ahead); m->logits = (float*)(b + o_logits); m->amax = (float4*)(b + o_amax);
            m->part = (float*)(b + o_part); m->rope_cs = (float2*)(b + o_rope);
            m->kcache = (T*)(b + o_k); m->vcache = (T*)(b + o_v);
            m->kv_len = (int*)(b + o_kvlen); m->next_token = (int*)(b + o_next); m->active_dev = (int*)(b + o_active); m->row_len = (int*)(b + o_rowlen);
            m->out_token = (int*)(b + o_out);
            m->out_score = (float*)(m->out_token + (size_t)SA_MAX_STEPS * S);
            m->out_bbox = (int*)(m->out_score + (size_t)SA_MAX_STEPS * S);
            m->out_bytes = (size_t)SA_MAX_STEPS * S * 8 * sizeof(int);
        }
        return cv.off;
    }

    int init(const surya_rec_config& cfg, const void* const* weights, int n) {
        c = cfg;
        w.assign(weights, weights + n);
        arena_bytes = layout(c, nullptr);
        for (auto& o : outs) o.slots = c.max_slots;
        const size_t mirror = (size_t)SA_MAX_STEPS * c.max_slots * 32;      // the base set's cells: token 4, score 4, box 24 bytes
        int rc = blk[B_MAIN].alloc(arena_bytes, mirror, 0, {}, false);       // memory as it comes: every buffer is written before it is read
        if (rc) return rc;
        poison_arena(blk[B_MAIN].dev, arena_bytes);
        layout(c, this);
        if ((rc = launch_rope_table<T>(reinterpret_cast<const float*>(w[SA_RW_DEC_INVFREQ]), rope_cs, c.max_kv_len, c.dec_head_dim / 2, 0))) return rc;
        SA_HIP(hipMemset(kv_len, 0, c.max_slots * sizeof(int)));
        SA_HIP(hipMemset(next_token, 0, c.max_slots * sizeof(int)));
        SA_HIP(hipMemset(out_token, 0, out_bytes));
        StepOutputs& base = outs[STEPS_BASE];              // always on: a ring half counts as mirrored from the start
        base.add(out_token, 4); base.add(out_score, 4); base.add(out_bbox, 24);
        base.mirrored[0] = base.mirrored[1] = true;
        base.host = blk[B_MAIN].host;                      // (the other sets' mirrors come with their blocks, too)
        if (base.host_bytes() != mirror) return SA_ERR_STATE;
        const size_t Pm = c.max_patches, Tm = std::max(c.max_prefill_tokens, c.max_slots);
        rc = st.init((Pm * 8 + Tm * 8 + (size_t)c.max_slots * 64) * sizeof(int) + (1 << 20));
        if (rc) return rc;
        rc = st_small.init((size_t)c.max_slots * 4 * sizeof(int) + 4096);
        if (rc) return rc;
        rc = st_enc.init((Pm * 8 + (size_t)c.max_slots * 64) * sizeof(int) + (1 << 20));
        if (rc) return rc;
        {   // the look-ahead encoder runs beside the decode steps: lowest priority, so decode kernels get CUs first
            int least = 0, greatest = 0;
            SA_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
            // (confining the encoder to a CU mask instead -- 128 / 192 / 224 CUs, prefix or strided -- was measured and is
            // slower than priority alone: 2599-2719 vs 2799 lines/s on 1024 lines, r01)
            SA_HIP(hipStreamCreateWithPriority(&estream, hipStreamNonBlocking, least));
            SA_HIP(hipEventCreateWithFlags(&ev_ahead_in, hipEventDisableTiming));
            SA_HIP(hipEventCreateWithFlags(&ev_ahead_done, hipEventDisableTiming));
            SA_HIP(hipEventCreateWithFlags(&ev_ahead_free, hipEventDisableTiming));
        }
        SA_HIP(hipStreamCreateWithFlags(&gstream, hipStreamNonBlocking));
        SA_HIP(hipEventCreateWithFlags(&gev_in, hipEventDisableTiming));
        SA_HIP(hipEventCreateWithFlags(&gev_out, hipEventDisableTiming));
        for (auto& e : ev_ring) SA_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        // hipGraph replay of the decode steps is opt-in (surya_set_tuning("graph", 1)): with the pipelined decode_async loop the host
        // enqueues call n + 1 while call n runs, so plain launches never starve the GPU, and a graph launch of ~450 kernel
        // nodes starts later than the first eager launch does (r01: 101.1 ms/step with graphs, 96.2 ms without).
        use_graph = true;                                  // cleared for good if a capture fails
        SA_HIP(hipDeviceSynchronize());
        return SA_OK;
    }

    // ------------------------------------------------------------------------------------------ helpers
    template <int EPI>
    int gemm(const T* X, long ldx, const T* Wt, long ldw, T* C, long ldc, const T* bias, const T* R, long ldr, int M, int N,
             int K, hipStream_t s) {
        GemmArgs<T, T> a{X, ldx, Wt, ldw, C, ldc, bias, R, ldr, M, N, K};
        return launch_gemm<T, T, EPI>(a, s);
    }
    int rmsnorm(const T* x, long ldx, const T* wt, T* y, long ldy, const int* src_row, int rows, int C, float eps, hipStream_t s) {
        return launch_rmsnorm<T>(x, ldx, wt, y, ldy, src_row, rows, C, eps, s);
    }

    // Vision encoder for images [0, n) whose tiles start at `tiles`; merged tokens (original order index g)
    // are written to dst + dst_rows[g] * dec_hidden. Chunks on image boundaries when P exceeds max_patches.
    int encode(const float* tiles, const int32_t* grid_hw, int n, const std::vector<int>& dst_rows, T* dst, hipStream_t s) {
        return encode(tiles, grid_hw, n, dst_rows, dst, s, st);
    }
    int encode(const float* tiles, const int32_t* grid_hw, int n, const std::vector<int>& dst_rows, T* dst, hipStream_t s,
               Stager& st) {
        const int unit = c.merge * c.merge, He = c.enc_hidden, D = He / c.enc_heads;
        int i0 = 0;
        long patch_base = 0, tok_base = 0;
        while (i0 < n) {
            int i1 = i0;
            long P = 0;
            while (i1 < n) {
                const long p = (long)grid_hw[2 * i1] * grid_hw[2 * i1 + 1];
                if (p > c.max_patches) return SA_ERR_SHAPE;
                if (P + p > c.max_patches) break;
                P += p; ++i1;
            }
            EncPlan pl;
            int rc = plan_encoder(c, grid_hw + 2 * i0, i1 - i0, pl);
            if (rc) return rc;
            SegLists win, full;
            for (size_t sgi = 0; sgi + 1 < pl.win_cu.size(); ++sgi) {
                const int a = pl.win_cu[sgi], L = pl.win_cu[sgi + 1] - a;
                win.seg_len.push_back(L);
                win.q_off.push_back((long)a * 3 * He); win.k_off.push_back((long)a * 3 * He + He);
                win.v_off.push_back((long)a * 3 * He + 2 * He); win.o_off.push_back((long)a * He);
                win.add_tiles((int)sgi, L);
            }
            for (size_t sgi = 0; sgi + 1 < pl.img_cu.size(); ++sgi) {
                const int a = pl.img_cu[sgi], L = pl.img_cu[sgi + 1] - a;
                full.seg_len.push_back(L);
                full.q_off.push_back((long)a * 3 * He); full.k_off.push_back((long)a * 3 * He + He);
                full.v_off.push_back((long)a * 3 * He + 2 * He); full.o_off.push_back((long)a * He);
                full.add_tiles((int)sgi, L);
            }
            std::vector<int> dst_row(pl.merged_src.size());
            for (size_t g = 0; g < dst_row.size(); ++g) dst_row[g] = dst_rows[tok_base + pl.merged_src[g]];
            st.begin();
            const int* d_src_row = st.put(pl.src_row);
            const int* d_pos = st.put(pl.pos_hw);
            const int* d_dst = st.put(dst_row);
            const int* d_hidx = st.put(pl.hidx);
            const int* d_widx = st.put(pl.widx);
            AttnSegs d_win = stage_segs(st, win), d_full = stage_segs(st, full);
            if (!d_full.o_off) return SA_ERR_NOMEM;
            rc = st.flush(s);
            if (rc) return rc;

            const int Pi = (int)P;
            if ((rc = launch_convert_tiles<T>(tiles + patch_base * c.patch_dim, tiles_t, d_src_row, Pi, c.patch_dim, c.patch_dim_pad, s))) return rc;
            if ((rc = gemm<EPI_BIAS>(tiles_t, c.patch_dim_pad, W(SA_RW_PATCH), c.patch_dim_pad, ex, He, nullptr, nullptr, 0, Pi,
                                     He, c.patch_dim_pad, s))) return rc;
            const float scale = 1.0f / sqrtf((float)D);
            if ((rc = launch_rope_vision_table(d_pos, reinterpret_cast<const float*>(w[SA_RW_ENC_INVFREQ]), erope, Pi, D, s))) return rc;
            for (int l = 0; l < c.enc_depth; ++l) {
                if ((rc = rmsnorm(ex, He, WE(l, SA_RE_NORM1), eh, He, nullptr, Pi, He, c.enc_eps, s))) return rc;
                {   // qkv projection with the 2-D rotary embedding of q and k in its epilogue (pair-interleaved weight rows)
                    GemmArgs<T, T> a{eh, He, WE(l, SA_RE_QKV_W), He, eqkv, 3 * He, WE(l, SA_RE_QKV_B), nullptr, 0, Pi, 3 * He, He};
                    a.rope = erope; a.rope_cols = 2 * He; a.rope_D = D;
                    if ((rc = launch_gemm<T, T, EPI_ROPE>(a, s))) return rc;
                }
                const bool fullatt = (c.fullatt_mask >> l) & 1u;
                const AttnSegs& sg = fullatt ? d_full : d_win;
                const int nt = (int)(fullatt ? full.tile_seg.size() : win.tile_seg.size());
                if ((rc = launch_attn<T>(D, eqkv, eqkv, eqkv, eh, sg, nt, c.enc_heads, 3 * He, D, 3 * He, D, He, D, 1, 0, scale, s)))
                    return rc;
                if ((rc = gemm<EPI_RESIDUAL>(eh, He, WE(l, SA_RE_PROJ_W), He, ex, He, WE(l, SA_RE_PROJ_B), ex, He, Pi, He, He, s)))
                    return rc;
                if ((rc = rmsnorm(ex, He, WE(l, SA_RE_NORM2), eh, He, nullptr, Pi, He, c.enc_eps, s))) return rc;
                if ((rc = gemm<EPI_SWIGLU>(eh, He, WE(l, SA_RE_GU_W), He, emlp, c.enc_inter_pad, WE(l, SA_RE_GU_B), nullptr, 0,
                                           Pi, 2 * c.enc_inter_pad, He, s))) return rc;
                if ((rc = gemm<EPI_RESIDUAL>(emlp, c.enc_inter_pad, WE(l, SA_RE_DOWN_W), c.enc_inter_pad, ex, He,
                                             WE(l, SA_RE_DOWN_B), ex, He, Pi, He, c.enc_inter_pad, s))) return rc;
            }
            // merger: ln_q eps is fixed 1e-6 in the reference (encoder/__init__.py:114)
            if ((rc = rmsnorm(ex, He, W(SA_RW_MERGER_LN), eh, He, nullptr, Pi, He, 1e-6f, s))) return rc;
            const int Mg = Pi / unit, Hm = He * unit;
            if ((rc = gemm<EPI_GELU>(eh, Hm, W(SA_RW_FC1_W), Hm, emh, Hm, W(SA_RW_FC1_B), nullptr, 0, Mg, Hm, Hm, s))) return rc;
            if ((rc = gemm<EPI_BIAS>(emh, Hm, W(SA_RW_FC2_W), Hm, emerged, c.enc_out_hidden, W(SA_RW_FC2_B), nullptr, 0, Mg,
                                     c.enc_out_hidden, Hm, s))) return rc;
            if ((rc = launch_scatter_image<T>(emerged, W(SA_RW_IMG_H), W(SA_RW_IMG_W), d_dst, d_hidx, d_widx, dst, Mg, c.dec_hidden, s))) return rc;
            patch_base += P;
            tok_base += P / unit;
            i0 = i1;
        }
        return SA_OK;
    }

    int encode_only(const float* tiles, const int32_t* grid_hw, int n, void* out, hipStream_t s) override {
        if (c.enc_out_hidden != c.dec_hidden) return SA_ERR_SHAPE;
        long ntok = 0;
        for (int i = 0; i < n; ++i) ntok += (long)grid_hw[2 * i] * grid_hw[2 * i + 1] / (c.merge * c.merge);
        std::vector<int> ident(ntok);
        for (long i = 0; i < ntok; ++i) ident[i] = (int)i;
        return encode(tiles, grid_hw, n, ident, reinterpret_cast<T*>(out), s);
    }

    // Look-ahead encoding: the vision encoder needs no KV slots, so the images of the NEXT lines in the queue are encoded on
    // a second (low-priority) stream while the current lines decode -- the decode phase is a chain of short latency-bound
    // kernels that leaves most of the chip idle (two bench processes on one GPU: 3149 vs 2727 lines/s, r01). The embeddings
    // land in emb_ahead in image order; prefill(tiles = NULL, ...) consumes them front to back.
    int encode_ahead(const float* tiles, const int32_t* grid_hw, int n, hipStream_t s) override {
        if (c.enc_out_hidden != c.dec_hidden) return SA_ERR_SHAPE;
        if (n == 0) {                                                    // discard: a caller whose loop ended early (an exception between
            ahead_consumed = ahead_tokens = 0;                           // encode_ahead and the prefill that would have consumed it) starts clean;
            return SA_OK;                                                // emb_ahead is re-used only behind ev_ahead_free / stream order as always
        }
        if (n < 0 || !tiles || !grid_hw) return SA_ERR_ARG;
        if (ahead_consumed != ahead_tokens) return SA_ERR_STATE;         // previous look-ahead not fully consumed
        long ntok = 0;
        for (int i = 0; i < n; ++i) ntok += (long)grid_hw[2 * i] * grid_hw[2 * i + 1] / (c.merge * c.merge);
        if (ntok > std::max(c.max_prefill_tokens, c.max_slots)) return SA_ERR_SHAPE;
        std::vector<int> ident(ntok);
        for (long i = 0; i < ntok; ++i) ident[i] = (int)i;
        SA_HIP(hipEventRecord(ev_ahead_in, s));                          // tiles were produced on the caller's stream
        SA_HIP(hipStreamWaitEvent(estream, ev_ahead_in, 0));
        if (ahead_free_recorded) SA_HIP(hipStreamWaitEvent(estream, ev_ahead_free, 0));   // last consumer of emb_ahead is done
        int rc = encode(tiles, grid_hw, n, ident, emb_ahead, estream, st_enc);
        if (rc) return rc;
        SA_HIP(hipEventRecord(ev_ahead_done, estream));
        ahead_tokens = ntok;
        ahead_consumed = 0;
        return SA_OK;
    }

    // ------------------------------------------------------------------------------------------ decoder
    // Prefill: packed prompt tokens, causal attention over the freshly written cache rows.
    int decoder_layers_prefill(int M, const int* d_tok_slot, const int* d_tok_pos, const AttnSegs* sg, int n_tiles, hipStream_t s) {
        const int Hd = c.dec_hidden, nq = c.dec_heads, nkv = c.dec_kv_heads, d = c.dec_head_dim, I = c.dec_inter;
        const int qkv_d = (nq + 2 * nkv) * d;
        const float scale = 1.0f / sqrtf((float)d);
        const size_t layer_kv = (size_t)c.max_slots * nkv * c.max_kv_len * d;
        const float* inv_freq = reinterpret_cast<const float*>(w[SA_RW_DEC_INVFREQ]);
        int rc;
        for (int l = 0; l < c.dec_layers; ++l) {
            T* kc = kcache + l * layer_kv;
            T* vc = vcache + l * layer_kv;
            if ((rc = rmsnorm(dx, Hd, WD(l, SA_RD_LN1), dh, Hd, nullptr, M, Hd, c.dec_eps, s))) return rc;
            if ((rc = gemm<EPI_BIAS>(dh, Hd, WD(l, SA_RD_QKV_W), Hd, dqkv, qkv_d, WD(l, SA_RD_QKV_B), nullptr, 0, M, qkv_d, Hd, s)))
                return rc;
            if ((rc = launch_rope_kv_append<T>(dqkv, d_tok_slot, d_tok_pos, rope_cs, kc, vc, M, nq, nkv, d, c.max_kv_len, s))) return rc;
            if constexpr (std::is_same<T, bf16_t>::value) {
                if (kv8) {
                    const size_t l8 = (size_t)c.max_slots * nkv, T8 = tmax8();
                    if ((rc = launch_kv8_quant_rows(d, kc, vc, d_tok_slot, d_tok_pos, M, k8c + l * l8 * c.max_kv_len * d, v8tc + l * l8 * d * T8,
                                                    ksc8 + l * l8 * T8, vsc8 + l * l8 * T8, nkv, c.max_kv_len, s))) return rc;
                }
            }
            if ((rc = launch_attn<T>(d, dqkv, kc, vc, dattn, *sg, n_tiles, nq, qkv_d, d, d, (long)c.max_kv_len * d, (long)nq * d, d,
                                     nq / nkv, 1, scale, s))) return rc;
            if ((rc = gemm<EPI_RESIDUAL>(dattn, (long)nq * d, WD(l, SA_RD_O_W), (long)nq * d, dx, Hd, nullptr, dx, Hd, M, Hd, nq * d,
                                         s))) return rc;
            if ((rc = rmsnorm(dx, Hd, WD(l, SA_RD_LN2), dh, Hd, nullptr, M, Hd, c.dec_eps, s))) return rc;
            if ((rc = gemm<EPI_SWIGLU>(dh, Hd, WD(l, SA_RD_GU_W), Hd, dmlp, I, nullptr, nullptr, 0, M, 2 * I, Hd, s))) return rc;
            if ((rc = gemm<EPI_RESIDUAL>(dmlp, I, WD(l, SA_RD_DOWN_W), I, dx, Hd, nullptr, dx, Hd, M, Hd, I, s))) return rc;
        }
        return SA_OK;
    }

    // The rows of a decode step and their workspaces: every per-row buffer is row-major, so a row range is a pointer offset.
    // (r02 ran two halves of the batch on two streams: no gain -- a 128-row launch takes as long as a 256-row one -- removed.)
    struct Half { int r0, M; float* part; hipStream_t s; };

    int splitk_gemm(const T* X, long ldx, const T* Wt, long ldw, int M, int N, int K, float* part_, int* S, hipStream_t s) {
        GemmArgs<T, T> a{X, ldx, Wt, ldw, nullptr, 0, nullptr, nullptr, 0, M, N, K, 1, part_};
        int rc = launch_gemm_splitk<T>(a, s);
        *S = a.splitk;
        return rc;
    }
    // pf_cache: the K or V cache of the layer whose decode attention comes next -- M extra workgroups request this step's rows of it
    // while the reduce runs (KvPrefetch, kernels.h). bf16 cache only; nullptr = plain reduce.
    int reduce_residual_norm(int S, int M, const float* part_, T* x, const T* wnorm, T* y, hipStream_t s, uint8_t* y8 = nullptr,
                             uint8_t* sy = nullptr, const T* pf_cache = nullptr, const Half* h = nullptr) {
        KvPrefetch pf;
        if (pf_cache && h && tuning().kvprefetch && (c.dec_head_dim * sizeof(T)) % 16 == 0) {
            pf.base = reinterpret_cast<const unsigned char*>(pf_cache);
            pf.slots = active_dev + h->r0; pf.lens = row_len + h->r0;
            pf.head_stride = (long)c.max_kv_len * c.dec_head_dim * sizeof(T);
            pf.slot_stride = pf.head_stride * c.dec_kv_heads;
            pf.heads = c.dec_kv_heads; pf.row_bytes = c.dec_head_dim * (int)sizeof(T); pf.max_rows = c.max_kv_len;
        }
        return launch_reduce_norm<T>(part_, S, M, x, wnorm, y, c.dec_hidden, c.dec_eps, y8, sy, c.max_slots, pf, s);
    }

    // FP8 KV cache for the decode steps (bf16 model only). Takes effect for lines prefilled AFTER the call: switch while no line
    // is in flight.
    int set_kv_fp8(int on) override {
        if constexpr (!std::is_same<T, bf16_t>::value) return on ? SA_ERR_UNSUPPORTED : SA_OK;
        if (on && excluded(M_KV8)) return SA_ERR_STATE;
        if ((on != 0) != kv8) drop_graphs();
        if (!on) { kv8 = false; return SA_OK; }
        const int d = c.dec_head_dim;
        if (d != 128 && d != 64 && d != 32) return SA_ERR_UNSUPPORTED;
        if (c.dec_heads / c.dec_kv_heads > 8) return SA_ERR_UNSUPPORTED;
        if (!blk[B_KV8].dev) {
            const size_t rows = (size_t)c.dec_layers * c.max_slots * c.dec_kv_heads, T8 = tmax8();
            Carve cv;
            const size_t o_k = cv.take(rows * c.max_kv_len * d), o_v = cv.take(rows * d * T8), o_ks = cv.take(rows * T8 * 4), o_vs = cv.take(rows * T8 * 4);
            const int rc = blk[B_KV8].alloc(cv.off);        // zeroed: finite bytes and scales everywhere, masked key columns multiply P = 0
            if (rc) return rc;
            char* b = blk[B_KV8].dev;
            k8c = (uint8_t*)(b + o_k); v8tc = (uint8_t*)(b + o_v);
            ksc8 = (float*)(b + o_ks); vsc8 = (float*)(b + o_vs);
        }
        kv8 = true;
        return SA_OK;
    }

    // Selection and fork of one step for `n_groups` groups: lead slots at list[g * stride] (beam.h). first: the prefill's selection.
    int beam_step(const int* list, int stride, int n_groups, int step, int first, hipStream_t s) {
        const size_t so = (size_t)step * c.max_slots;
        BeamSelectArgs a{list, stride, n_groups, beam, c.max_slots, alt_token + so * SA_MAX_ALTERNATIVES, alt_prob + so * SA_MAX_ALTERNATIVES,
                         beam_score, beam_fin, c.eos_token_id, c.pad_token_id, beam_nop, first, beam_token + so, beam_parent + so, beam_rank + so,
                         beam_prob + so, beam_logp + so, next_token, fork_src, kv_len, beam_prompt, fork_base, fork_len, c.max_kv_len};
        GemmProfiler& pf = gemm_profiler();                   // surya_prof_enable: the two launches as buckets 4 and 5 (time only)
        auto timed = [&](int bucket, auto&& launch) -> int {
            const bool prof = pf.enabled && pf.n < GemmProfiler::POOL;
            if (prof) (void)hipEventRecord(pf.ev[2 * pf.n], s);
            const int rc = launch();
            if (prof) {
                (void)hipEventRecord(pf.ev[2 * pf.n + 1], s);
                pf.cfg_of[pf.n] = bucket; pf.flops_of[pf.n] = pf.bytes_of[pf.n] = pf.slab_of[pf.n] = 0.0;
                ++pf.n;
            }
            return rc;
        };
        int rc = timed(4, [&] { return launch_beam_select(a, s); });
        if (rc) return rc;
        return timed(5, [&] {
            return launch_kv_fork<T>(kcache, vcache, list, stride == 1 ? beam : 1, fork_src, fork_base, fork_len, n_groups * beam, c.dec_layers,
                                     c.max_slots, c.dec_kv_heads, c.max_kv_len, c.dec_head_dim, s);
        });
    }

    // MXFP8 weight table of the decode steps: per layer SA_MX_COUNT pointers, then SA_MX_LM_W, SA_MX_LM_S. bf16 model only.
    int set_mx_weights(const void* const* tbl, int n) override {
        if constexpr (!std::is_same<T, bf16_t>::value) return SA_ERR_UNSUPPORTED;
        if (!tbl) { if (!mxw.empty()) drop_graphs(); mxw.clear(); return SA_OK; }     // back to the bf16 decode weights
        if (excluded(M_MX)) return SA_ERR_STATE;
        if (n != SA_MX_TOTAL(c.dec_layers)) return SA_ERR_ARG;
        for (int i = 0; i < n; ++i)
            if (!tbl[i]) return SA_ERR_ARG;
        const int Hd = c.dec_hidden, A = c.dec_heads * c.dec_head_dim, I = c.dec_inter;
        if (Hd % 128 || A % 128 || I % 128 || c.dec_head_dim % 32) return SA_ERR_SHAPE;     // whole 128-element K-tiles, 32-wide blocks
        if (!blk[B_MX].dev) {
            const size_t S = c.max_slots;
            Carve cv;
            const size_t o1 = cv.take(S * Hd), o2 = cv.take(S * Hd / 32), o3 = cv.take(S * A), o4 = cv.take(S * A / 32), o5 = cv.take(S * I),
                         o6 = cv.take(S * I / 32), o7 = cv.take(S * Hd), o8 = cv.take(S * Hd / 32);
            const int rc = blk[B_MX].alloc(cv.off);
            if (rc) return rc;
            uint8_t* b = reinterpret_cast<uint8_t*>(blk[B_MX].dev);
            dh8 = b + o1; sdh = b + o2; dattn8 = b + o3; sattn = b + o4; dmlp8 = b + o5; smlp = b + o6; dlast8 = b + o7; slast = b + o8;
        }
        mxw.resize(n);
        for (int i = 0; i < n; ++i) mxw[i] = reinterpret_cast<const uint8_t*>(tbl[i]);
        drop_graphs();                                                  // captured steps hold the old launch arguments
        return SA_OK;
    }

    int decode_embed(const Half& h) {
        const int Hd = c.dec_hidden;
        return launch_decode_embed<T>(W(SA_RW_TOK_EMBED), next_token, active_dev + h.r0, kv_len, c.max_kv_len, row_len + h.r0, dx + (size_t)h.r0 * Hd,
                                      WD(0, SA_RD_LN1), dh + (size_t)h.r0 * Hd, h.M, Hd, c.dec_eps, mx() ? dh8 + (size_t)h.r0 * Hd : nullptr,
                                      mx() ? sdh + (size_t)h.r0 * 4 : nullptr, c.max_slots, mx(), h.s);
    }

    // One decoder layer of one decode step for the rows of `h`. The three skinny projections (qkv, o, down) run split-K so
    // they cover the chip; their partial sums are combined by the kernel that needs the result anyway: decode attention
    // (qkv) and a fused residual-add + next-RMSNorm pass (o, down). The last layer leaves the final-norm rows in `dlast`.
    int decode_layer(int l, const Half& h) {
        const int Hd = c.dec_hidden, nq = c.dec_heads, nkv = c.dec_kv_heads, d = c.dec_head_dim, I = c.dec_inter;
        const int qkv_d = (nq + 2 * nkv) * d, M = h.M;
        const float scale = 1.0f / sqrtf((float)d);
        const size_t layer_kv = (size_t)c.max_slots * nkv * c.max_kv_len * d;
        hipStream_t s = h.s;
        T* kc = kcache + l * layer_kv;
        T* vc = vcache + l * layer_kv;
        T* x = dx + (size_t)h.r0 * Hd;
        T* hh = dh + (size_t)h.r0 * Hd;
        T* at = dattn + (size_t)h.r0 * nq * d;
        T* ml = dmlp + (size_t)h.r0 * I;
        const int* act = active_dev + h.r0;
        const int* rl = row_len + h.r0;
        int rc, S = 1;
        const bool q8 = mx();
        const int A = nq * d;
        uint8_t *hh8 = nullptr, *shh = nullptr, *at8 = nullptr, *sat = nullptr, *ml8 = nullptr, *sml = nullptr;
        if (q8) {
            hh8 = dh8 + (size_t)h.r0 * Hd; shh = sdh + (size_t)h.r0 * 4;
            at8 = dattn8 + (size_t)h.r0 * A; sat = sattn + (size_t)h.r0 * 4;
            ml8 = dmlp8 + (size_t)h.r0 * I; sml = smlp + (size_t)h.r0 * 4;
        }
        rc = -1;
        if constexpr (MX_OK) {
            if (q8) rc = splitk_gemm_mx(hh8, shh, Hd, MXW(l, SA_MX_QKV_W), MXW(l, SA_MX_QKV_S), M, qkv_d, Hd, h.part, &S, s);
        }
        if (!q8) rc = splitk_gemm(hh, Hd, WD(l, SA_RD_QKV_W), Hd, M, qkv_d, Hd, h.part, &S, s);
        if (rc) return rc;
        bool launched = false;
        if constexpr (std::is_same<T, bf16_t>::value) {
            if (kv8) {                                       // FP8 KV cache (decode_attn_kv8.h)
                const size_t l8 = (size_t)c.max_slots * nkv, T8 = tmax8();
                DecodeAttnKv8Args a{h.part, S, WD(l, SA_RD_QKV_B), at, k8c + l * l8 * c.max_kv_len * d, v8tc + l * l8 * d * T8, ksc8 + l * l8 * T8,
                                    vsc8 + l * l8 * T8, act, rl, rope_cs, M, nq, nkv, d, c.max_kv_len, scale, at8, sat, c.max_slots};
                if ((rc = launch_decode_attn_kv8(a, s))) return rc;
                launched = true;
            }
        }
        if (!launched) {
            DecodeAttnArgs<T> a{h.part, S, WD(l, SA_RD_QKV_B), at, kc, vc, act, rl, rope_cs, M, nq, nkv, d, c.max_kv_len, scale, ctx_bound, at8, sat,
                                c.max_slots};
            if ((rc = launch_decode_attn<T>(a, s))) return rc;
        }
        const bool last = (l + 1 == c.dec_layers);
        const T* wnext = last ? W(SA_RW_DEC_NORM) : WD(l + 1, SA_RD_LN1);
        T* ynext = last ? dlast + (size_t)h.r0 * Hd : hh;
        if constexpr (MX_OK) if (q8) {
            if ((rc = splitk_gemm_mx(at8, sat, A, MXW(l, SA_MX_O_W), MXW(l, SA_MX_O_S), M, Hd, A, h.part, &S, s))) return rc;
            if ((rc = reduce_residual_norm(S, M, h.part, x, WD(l, SA_RD_LN2), hh, s, hh8, shh))) return rc;
            MxArgs g{hh8, Hd, shh, MXW(l, SA_MX_GU_W), Hd, MXW(l, SA_MX_GU_S), M, 2 * I, Hd, (long)c.max_slots, (long)2 * I};
            g.Q = ml8; g.ldq = I; g.SQ = sml; g.sq_rows = c.max_slots;
            if ((rc = launch_gemm_mx<MX_EPI_SWIGLU>(g, s))) return rc;
            if ((rc = splitk_gemm_mx(ml8, sml, I, MXW(l, SA_MX_DOWN_W), MXW(l, SA_MX_DOWN_S), M, Hd, I, h.part, &S, s))) return rc;
            return reduce_residual_norm(S, M, h.part, x, wnext, ynext, s, last ? dlast8 + (size_t)h.r0 * Hd : hh8,
                                        last ? slast + (size_t)h.r0 * 4 : shh);
        }
        // the next layer's cache rows of this step's slots are requested while the two reduce kernels run: V first (it is needed
        // second and may fall back to the infinity cache behind gate|up's 26 MB), K right before the attention launch
        const bool warm = !last && !kv8;
        const T* v_next = warm ? vcache + (size_t)(l + 1) * layer_kv : nullptr;
        const T* k_next = warm ? kcache + (size_t)(l + 1) * layer_kv : nullptr;
        if ((rc = splitk_gemm(at, (long)nq * d, WD(l, SA_RD_O_W), (long)nq * d, M, Hd, nq * d, h.part, &S, s))) return rc;
        if ((rc = reduce_residual_norm(S, M, h.part, x, WD(l, SA_RD_LN2), hh, s, nullptr, nullptr, v_next, &h))) return rc;
        if ((rc = gemm<EPI_SWIGLU>(hh, Hd, WD(l, SA_RD_GU_W), Hd, ml, I, nullptr, nullptr, 0, M, 2 * I, Hd, s))) return rc;
        if ((rc = splitk_gemm(ml, I, WD(l, SA_RD_DOWN_W), I, M, Hd, I, h.part, &S, s))) return rc;
        return reduce_residual_norm(S, M, h.part, x, wnext, ynext, s, nullptr, nullptr, k_next, &h);
    }

    // fuse_next: the rows are the active list of a decode call and another step follows -- the head also writes that step's
    // embedding, first RMSNorm and row_len (decode_eager skips the embed launch).
    // xrows: the pre-norm rows d_last_row indexes, where they are not the prefill's (restore: the store's hidden rows).
    int heads(int rows, const int* d_last_row, const int* d_row_slot, int step, int len_inc, bool normed, hipStream_t s, bool fuse_next = false,
              const T* xrows = nullptr) {
        const int Hd = c.dec_hidden;
        int rc;
        T* last = dlast;
        float4* am = amax;
        if (!normed && (rc = rmsnorm(xrows ? xrows : dx, Hd, W(SA_RW_DEC_NORM), last, Hd, d_last_row, rows, Hd, c.dec_eps, s))) return rc;
        // lm_head with the greedy reduction in its epilogue: logits stay in LDS, the head combines per-tile partials.
        // Which greedy epilogue the mode asks for -- forced | candidates (masked or not) | masked | plain -- and what it reads, once for
        // both weight formats: `launch(a, tag)` runs `a` with epilogue EPIS[tag] of its format.
        int bn_used = 0;
        auto lm_head = [&](auto& a, auto&& launch) -> int {
            a.amax = am;
            if (forcing) {
                a.forced = forced_cols(d_row_slot);
            } else {
                if (n_token_masks > 0) a.tmask = token_mask(d_row_slot);
                if (topk()) a.alt = alt_part;
            }
            const int rc_ =forcing ? launch(a, HeadEpi<0>{}) : topk() ? launch(a, HeadEpi<1>{}) : n_token_masks > 0 ? launch(a, HeadEpi<2>{}) : launch(a, HeadEpi<3>{});
            bn_used = a.bn_used;
            if (rc_ || bst_states == 0) return rc_;
            // boosted decoding: that was record A (the masked epilogue; a boosted slot's row is its preferred set). Record B, the plain
            // greedy epilogue of the same tiling, goes into the second partial buffer.
            a.amax = amax_b;
            a.tmask = TokenMask{};
            const int rc_b = launch(a, HeadEpi<3>{});
            return rc_b ? rc_b : a.bn_used != bn_used ? (int)SA_ERR_STATE : (int)SA_OK;
        };
        if (mx() && normed) {       // decode steps: MXFP8 lm_head on the MXFP8 copy of the final-norm rows
            if constexpr (std::is_same<T, bf16_t>::value) {
                static constexpr int EPIS[4] = {MX_EPI_FORCED, MX_EPI_TOPK, MX_EPI_ARGMAX_MASK, MX_EPI_ARGMAX};
                MxArgs a{dlast8, Hd, slast, MXG(SA_MX_LM_W), Hd, MXG(SA_MX_LM_S), rows, c.vocab, Hd, (long)c.max_slots, (long)c.vocab};
                a.bias = W(SA_RW_LM_B);
                if ((rc = lm_head(a, [&](MxArgs& a_, auto e) { return launch_gemm_mx<EPIS[decltype(e)::value]>(a_, s); }))) return rc;
            }
        } else {
            static constexpr int EPIS[4] = {EPI_FORCED, EPI_TOPK, EPI_ARGMAX_MASK, EPI_ARGMAX};
            GemmArgs<T, float> a{last, Hd, W(SA_RW_LM_W), Hd, logits, c.vocab, W(SA_RW_LM_B), nullptr, 0, rows, c.vocab, Hd};
            if ((rc = lm_head(a, [&](GemmArgs<T, float>& a_, auto e) { return launch_gemm<T, float, EPIS[decltype(e)::value]>(a_, s); }))) return rc;
        }
        const int tiles_n = cdiv(c.vocab, bn_used);
        const size_t so = (size_t)step * c.max_slots;
        last_rows = rows;
        last_heads_mx = mx() && normed;
        float2* bt = topk() ? best_tot : nullptr;
        ForcedHead fh;                                        // empty while forcing is off: the heads do what they always did
        if (forcing) fh = ForcedHead{forced_table, forced_cursor, flogit, SA_MAX_FORCED_TOKENS, greedy_token + so, greedy_prob + so, forced_logprob + so};
        // alternatives: the row's four best candidates and their probabilities, behind whichever head ran
        auto combine = [&]() -> int {
            if ((rc = (int)hipGetLastError()) || !topk()) return rc;
            hipLaunchKernelGGL(topk_combine_kernel, dim3(rows), dim3(SA_ALT_THREADS), 0, s, alt_part, tiles_n, d_row_slot, bt,
                               alt_token + so * SA_MAX_ALTERNATIVES, alt_prob + so * SA_MAX_ALTERNATIVES);
            return (int)hipGetLastError();
        };
        const bool fz = fuse_next;
        HeadArgs<T> ha{reinterpret_cast<const float4*>(am), tiles_n, rows, last, Hd, W(SA_RW_BBOX_W), W(SA_RW_BBOX_B), d_row_slot, c.eos_token_id,
                       c.pad_token_id, (float)c.bbox_size, out_token + so, out_score + so, out_bbox + so * 6, next_token, kv_len, len_inc};
        ha.table = fz ? W(SA_RW_TOK_EMBED) : (const T*)nullptr;
        ha.wnorm = WD(0, SA_RD_LN1); ha.x = dx; ha.y = dh; ha.row_len = row_len; ha.Tmax = c.max_kv_len; ha.eps = c.dec_eps;
        ha.y8 = (fz && mx()) ? dh8 : (uint8_t*)nullptr; ha.sy = (fz && mx()) ? sdh : (uint8_t*)nullptr; ha.srows = c.max_slots;
        ha.best_tot = bt; ha.fh = fh;
        if (pat_states > 0)                                   // empty while patterns are off: the heads do what they always did
            ha.ph = PatternHead{pat_tok_class, pat_next_state, pat_state_mask, SA_MAX_PATTERN_CLASSES, c.vocab, slot_state, slot_mask};
        if (bst_states > 0) {                                 // boosted decoding: the head on both records, then every boosted slot's next state and row
            BoostHeadArgs<T> bh{ha, reinterpret_cast<const float4*>(amax_b), slot_bst_beta, plain_token + so, plain_prob + so};
            if ((rc = launch_boost_head<T>(bh, mx(), s))) return rc;
            return launch_boost_step(bst_args(), d_row_slot, out_token + so, rows, s);
        }
        if ((rc = launch_head<T>(ha, mx(), s))) return rc;
        // lexicon-guided decoding: behind the token, every lexicon slot's own mask row becomes its next state's allowed set (lexicon.h)
        if (lex_states > 0 && (rc = launch_lexicon_step(lex_args(), d_row_slot, out_token + so, rows, s))) return rc;
        return combine();
    }

    int prefill(const float* tiles, const int32_t* grid_hw, int n_images, const int32_t* input_ids, const int32_t* seq_offsets,
                const int32_t* slot_ids, int n_seqs, hipStream_t s) override {
        return prefill_fan(tiles, grid_hw, n_images, input_ids, seq_offsets, slot_ids, n_seqs, nullptr, nullptr, s);
    }

    // surya_rec_prefill_shared: sequence i is prefilled once, into its lead slot fan_slots[fan_offsets[i]], and then occupies every slot of
    // fan_slots[fan_offsets[i] .. fan_offsets[i + 1]). Everything about the fans is checked here, before anything is enqueued or changed.
    int prefill_shared(const float* tiles, const int32_t* grid_hw, int n_images, const int32_t* input_ids, const int32_t* seq_offsets,
                       const int32_t* fan_offsets, const int32_t* fan_slots, int n_seqs, hipStream_t s) override {
        if (n_seqs <= 0) return SA_OK;
        if (n_seqs > c.max_slots) return SA_ERR_ARG;
        if (beam > 0 || kv8) return SA_ERR_STATE;           // beam search owns whole groups and forks on its own; the fan-out copies no fp8 rows
        if (check_fans(fan_offsets, fan_slots, n_seqs, c.max_slots, [](int, int) { return true; })) return SA_ERR_ARG;
        std::vector<int32_t> leads(n_seqs);
        for (int i = 0; i < n_seqs; ++i) leads[i] = fan_slots[fan_offsets[i]];
        return prefill_fan(tiles, grid_hw, n_images, input_ids, seq_offsets, leads.data(), n_seqs, fan_offsets, fan_slots, s);
    }

    // ---------------------------------------------------------------------------------------- prompt store
    // Prompts that outlive their slots (surya_rec_prefill_keep / surya_rec_restore; kv_store.h): [K | V][layer][kv_head][store_cap][D] and
    // the hidden rows [store_cap][dec_hidden], in one lazily allocated block (B_STORE). RecBase holds the host's table of entries.
    // Decode steps never read the store, so no captured step holds one of its addresses and growing it drops none.
    T *store_k = nullptr, *store_v = nullptr, *store_h = nullptr;
    int reserve_prompts(int rows, hipStream_t s) override {
        if (rows < 0) return SA_ERR_ARG;
        if (rows <= store_cap) return SA_OK;
        const size_t runs = (size_t)c.dec_layers * c.dec_kv_heads, row_b = (size_t)c.dec_head_dim * sizeof(T), hid_b = (size_t)c.dec_hidden * sizeof(T);
        Carve cv;
        const size_t o_k = cv.take(runs * rows * row_b), o_v = cv.take(runs * rows * row_b), o_h = cv.take((size_t)rows * hid_b);
        DevBlock nb;
        int rc = nb.alloc(cv.off);
        if (rc) return rc;
        if (store_cap > 0) {     // every run's old rows to the front of its new run, in stream order; then nothing in flight reads the old block
            const size_t old_run = (size_t)store_cap * row_b, new_run = (size_t)rows * row_b;
            rc = (int)hipMemcpy2DAsync(nb.dev + o_k, new_run, store_k, old_run, old_run, runs, hipMemcpyDeviceToDevice, s);
            if (!rc) rc = (int)hipMemcpy2DAsync(nb.dev + o_v, new_run, store_v, old_run, old_run, runs, hipMemcpyDeviceToDevice, s);
            if (!rc) rc = (int)hipMemcpyAsync(nb.dev + o_h, store_h, (size_t)store_cap * hid_b, hipMemcpyDeviceToDevice, s);
        }
        if (!rc) rc = (int)hipDeviceSynchronize();
        if (rc) { nb.release(); return rc; }
        blk[B_STORE].release();
        blk[B_STORE] = nb;
        store_k = reinterpret_cast<T*>(nb.dev + o_k); store_v = reinterpret_cast<T*>(nb.dev + o_v); store_h = reinterpret_cast<T*>(nb.dev + o_h);
        store_cap = rows;
        return SA_OK;
    }
    // surya_rec_prefill_keep: the ranges are checked here, before anything is enqueued; the table changes once the launches are out.
    int prefill_keep(const float* tiles, const int32_t* grid_hw, int n_images, const int32_t* input_ids, const int32_t* seq_offsets,
                     const int32_t* slot_ids, int n_seqs, const int32_t* keep_first, hipStream_t s) override {
        if (n_seqs <= 0) return SA_OK;
        if (n_seqs > c.max_slots) return SA_ERR_ARG;
        if (kv8) return SA_ERR_STATE;                       // the store holds bf16 / fp16 / fp32 rows only
        std::map<int, int> live = store_live;
        if (check_keep(live, keep_first, seq_offsets, n_seqs, store_cap)) return SA_ERR_ARG;
        if (live.size() == store_live.size()) keep_first = nullptr;      // nothing named: surya_rec_prefill
        const int rc = prefill_fan(tiles, grid_hw, n_images, input_ids, seq_offsets, slot_ids, n_seqs, nullptr, nullptr, s, keep_first);
        if (!rc) store_live.swap(live);
        return rc;
    }
    // surya_rec_restore: restore_plan checks and stages everything, then the rows and the head pass.
    int restore(const int32_t* first, const int32_t* fan_offsets, const int32_t* fan_slots, int n, hipStream_t s) override {
        if (n <= 0) return SA_OK;
        RestorePlan p;
        int rc = restore_plan(first, fan_offsets, fan_slots, n, s, &p);
        if (rc) return rc;
        if ((rc = launch_kv_restore<T>(kcache, vcache, store_k, store_v, p.first, p.lens, p.foff, p.fslots, n, p.F, c.dec_layers, c.max_slots,
                                       c.dec_kv_heads, c.max_kv_len, c.dec_head_dim, store_cap, s))) return rc;
        if ((rc = heads(p.F, p.ffirst, p.fslots, 0, 0, false, s, false, store_h)) || beam == 0) return rc;
        return beam_step(p.fslots, 1, n, 0, 1, s);          // the B best first tokens, and the prompt's rows to the group's other slots
    }

    // The body of both prefills. fan_offsets == nullptr: surya_rec_prefill, one slot per sequence; with keep_first, surya_rec_prefill_keep.
    int prefill_fan(const float* tiles, const int32_t* grid_hw, int n_images, const int32_t* input_ids, const int32_t* seq_offsets,
                    const int32_t* slot_ids, int n_seqs, const int32_t* fan_offsets, const int32_t* fan_slots, hipStream_t s,
                    const int32_t* keep_first = nullptr) {
        if (n_seqs <= 0) return SA_OK;
        if (n_seqs > c.max_slots) return SA_ERR_ARG;
        const int Ttot = seq_offsets[n_seqs];
        if (Ttot > c.max_prefill_tokens) return SA_ERR_SHAPE;
        const int nq = c.dec_heads, nkv = c.dec_kv_heads, d = c.dec_head_dim;
        std::vector<int> ids(Ttot), tok_slot(Ttot), tok_pos(Ttot), lens(n_seqs), last_row(n_seqs), img_pos;
        SegLists sg;
        for (int i = 0; i < n_seqs; ++i) {
            const int a = seq_offsets[i], L = seq_offsets[i + 1] - a;
            if (L <= 0 || L >= c.max_kv_len || slot_ids[i] < 0 || slot_ids[i] >= c.max_slots) return SA_ERR_ARG;
            if (beam > 0 && (slot_ids[i] % beam || slot_ids[i] + beam > c.max_slots)) return SA_ERR_ARG;      // lead slots of whole groups only
            lens[i] = L; last_row[i] = a + L - 1;
            for (int t = 0; t < L; ++t) {
                const int id = input_ids[a + t];
                if (id < 0 || id >= c.vocab) return SA_ERR_ARG;
                const bool img = (id == c.image_token_id);
                ids[a + t] = img ? -1 : id;
                if (img) img_pos.push_back(a + t);
                tok_slot[a + t] = slot_ids[i]; tok_pos[a + t] = t;
            }
            sg.seg_len.push_back(L);
            sg.q_off.push_back((long)a * (nq + 2 * nkv) * d);
            sg.k_off.push_back((long)slot_ids[i] * nkv * c.max_kv_len * d);
            sg.v_off.push_back((long)slot_ids[i] * nkv * c.max_kv_len * d);
            sg.o_off.push_back((long)a * nq * d);
            sg.add_tiles(i, L);
        }
        long ntok = 0;
        for (int i = 0; i < n_images; ++i) ntok += (long)grid_hw[2 * i] * grid_hw[2 * i + 1] / (c.merge * c.merge);
        if ((long)img_pos.size() != ntok) return SA_ERR_SHAPE;   // reference only warns (common/surya/__init__.py:216-221)
        if (h_len.size() < (size_t)c.max_slots) h_len.resize(c.max_slots, 0);
        // The fans as the launches below take them: per fan slot its length and the prompt's last row (slot state, head pass), and per
        // sequence the slots behind the lead (kv_fanout_kernel).
        std::vector<int> f_lens, f_last, f_off, f_dst;
        for (int i = 0; i < n_seqs; ++i) {
            for (int b = 0; b < std::max(beam, 1); ++b) h_len[slot_ids[i] + b] = lens[i];
            if (!fan_offsets) continue;
            f_off.push_back((int)f_dst.size());
            for (int j = fan_offsets[i]; j < fan_offsets[i + 1]; ++j) {
                h_len[fan_slots[j]] = lens[i];
                f_lens.push_back(lens[i]); f_last.push_back(last_row[i]);
                if (j > fan_offsets[i]) f_dst.push_back(fan_slots[j]);
            }
        }
        if (fan_offsets) f_off.push_back((int)f_dst.size());
        int rc;
        // small plan first (its own stager: the encoder re-stages per chunk)
        st_small.begin();
        const int* d_slots = st_small.put(slot_ids, n_seqs);
        const int* d_lens = st_small.put(lens);
        const int* d_last = st_small.put(last_row);
        const int* d_keep = keep_first ? st_small.put(keep_first, n_seqs) : nullptr;
        if (!d_last || (keep_first && !d_keep)) return SA_ERR_NOMEM;
        if ((rc = st_small.flush(s))) return rc;
        // token embeddings for non-image positions
        {
            st.begin();
            const int* d_ids = st.put(ids);
            if (!d_ids) return SA_ERR_NOMEM;
            if ((rc = st.flush(s))) return rc;
            if ((rc = launch_embed_tokens<T>(W(SA_RW_TOK_EMBED), d_ids, dx, Ttot, c.dec_hidden, s))) return rc;
        }
        if (n_images > 0 && tiles) {
            if ((rc = encode(tiles, grid_hw, n_images, img_pos, dx, s))) return rc;
        } else if (n_images > 0) {
            // embeddings were encoded ahead (encode_ahead): take the next ntok rows of emb_ahead
            if (ahead_consumed + ntok > ahead_tokens) return SA_ERR_STATE;
            st.begin();
            const int* d_img = st.put(img_pos);
            if (!d_img) return SA_ERR_NOMEM;
            if ((rc = st.flush(s))) return rc;
            SA_HIP(hipStreamWaitEvent(s, ev_ahead_done, 0));
            if ((rc = launch_scatter_rows<T>(emb_ahead + ahead_consumed * c.dec_hidden, d_img, dx, (int)ntok, c.dec_hidden, s))) return rc;
            ahead_consumed += ntok;
            SA_HIP(hipEventRecord(ev_ahead_free, s));
            ahead_free_recorded = true;
        }
        st.begin();
        const int* d_tok_slot = st.put(tok_slot);
        const int* d_tok_pos = st.put(tok_pos);
        AttnSegs d_sg = stage_segs(st, sg);
        if (!d_sg.o_off) return SA_ERR_NOMEM;
        if (!fan_offsets) {
            if ((rc = st.flush(s))) return rc;
            hipLaunchKernelGGL(set_slot_state_kernel, dim3(cdiv(n_seqs, 256)), dim3(256), 0, s, d_slots, d_lens, kv_len, n_seqs);
            if ((rc = decoder_layers_prefill(Ttot, d_tok_slot, d_tok_pos, &d_sg, (int)sg.tile_seg.size(), s))) return rc;
            // kept prompts: their cache rows and the hidden row the head pass is about to read, while dx still holds it (kv_keep_kernel)
            if (keep_first && (rc = launch_kv_keep<T>(kcache, vcache, store_k, store_v, d_slots, d_keep, d_lens, n_seqs, c.dec_layers, c.max_slots,
                                                      c.dec_kv_heads, c.max_kv_len, c.dec_head_dim, store_cap, dx, d_last, store_h, c.dec_hidden,
                                                      Ttot, s))) return rc;
            if ((rc = heads(n_seqs, d_last, d_slots, 0, 0, false, s)) || beam == 0) return rc;
            return beam_step(d_slots, 1, n_seqs, 0, 1, s);   // the B best first tokens, and the prompt's rows to the group's other slots
        }
        // shared prefill: every fan slot gets the length and a head row of its own; the cache rows follow behind the layers
        const int F = fan_offsets[n_seqs], n_dst = (int)f_dst.size();
        const int* d_fslots = st.put(fan_slots, F);
        const int* d_flens = st.put(f_lens);
        const int* d_flast = st.put(f_last);
        const int* d_foff = st.put(f_off);
        if (f_dst.empty()) f_dst.push_back(-1);                 // (a call of single-slot fans: one entry nobody reads, n_dst stays 0)
        const int* d_fdst = st.put(f_dst);
        if (!d_fslots || !d_flens || !d_flast || !d_foff || !d_fdst) return SA_ERR_NOMEM;
        if ((rc = st.flush(s))) return rc;
        hipLaunchKernelGGL(set_slot_state_kernel, dim3(cdiv(F, 256)), dim3(256), 0, s, d_fslots, d_flens, kv_len, F);
        if ((rc = decoder_layers_prefill(Ttot, d_tok_slot, d_tok_pos, &d_sg, (int)sg.tile_seg.size(), s))) return rc;
        if ((rc = launch_kv_fanout<T>(kcache, vcache, d_slots, d_foff, d_fdst, d_lens, n_seqs, n_dst, c.dec_layers, c.max_slots, c.dec_kv_heads,
                                      c.max_kv_len, c.dec_head_dim, s))) return rc;
        return heads(F, d_flast, d_fslots, 0, 0, false, s);
    }

    int decode_eager(int M, int n_steps, int step0, hipStream_t s) {
        int rc;
        const Half h{0, M, part, s};
        const bool fuse = can_fuse_embed() && beam == 0;      // beam search: the next step's input is the selection's, not the head's
        if (h_len.size() < (size_t)c.max_slots) h_len.resize(c.max_slots, 0);
        for (int step = 0; step < n_steps; ++step) {
            ctx_bound = 0;
            for (int a : h_active) {
                ctx_bound = std::max(ctx_bound, h_len[a] + 1);
                h_len[a] = std::min(h_len[a] + 1, c.max_kv_len);
            }
            if ((step == 0 || !fuse) && (rc = decode_embed(h))) return rc;
            for (int l = 0; l < c.dec_layers; ++l)
                if ((rc = decode_layer(l, h))) return rc;
            if ((rc = heads(M, nullptr, active_dev, step0 + step, 1, true, s, fuse && step + 1 < n_steps))) return rc;
            if (beam > 0 && (rc = beam_step(active_dev, beam, M / beam, step0 + step, 0, s))) return rc;
        }
        return SA_OK;
    }

    int decode(int n_steps, hipStream_t s) override { return decode_steps(n_steps, 0, s); }

    // Pipelined form: the outputs of this call go to ring half `ring` (steps [8 * ring, 8 * ring + n_steps)) and are
    // mirrored to pinned host memory behind an event, so the caller can enqueue the NEXT call before it looks at this
    // one: the host-side bookkeeping and launch latency then overlap with the GPU instead of leaving it idle between
    // calls (r01 trace: ~0.7 ms idle per round trip, 8 % of the recognition step).
    int decode_async(int n_steps, int ring, hipStream_t s) override {
        if (n_steps < 0 || n_steps > SA_MAX_STEPS / 2 || ring < 0 || ring > 1) return SA_ERR_ARG;
        const int rc = decode_steps(n_steps, StepOutputs::ring_step(ring), s);
        return rc ? rc : mirror_steps(n_steps, ring, s);
    }

    int decode_steps(int n_steps, int step0, hipStream_t s) {
        if (n_steps < 0 || step0 < 0 || step0 + n_steps > SA_MAX_STEPS) return SA_ERR_ARG;
        const int M = n_active;
        if (M == 0 || n_steps == 0) return SA_OK;
        if (!use_graph || !tuning().graph || gemm_profiler().enabled) return decode_eager(M, n_steps, step0, s);
        if (graph_epoch != tuning_epoch()) { drop_graphs(); graph_epoch = tuning_epoch(); }   // a knob changed since the captures
        const long key = ((long)M * 64 + n_steps) * 64 + step0;
        auto it = graphs.find(key);
        if (it == graphs.end()) {
            // first sight of this shape runs eagerly (one-time hipFuncSetAttribute calls must not happen inside a capture)
            if (!seen_keys.count(key)) { seen_keys.insert(key); return decode_eager(M, n_steps, step0, s); }
            hipGraph_t g = nullptr;
            SA_HIP(hipStreamBeginCapture(gstream, hipStreamCaptureModeThreadLocal));
            int rc = decode_eager(M, n_steps, step0, gstream);
            hipError_t e = hipStreamEndCapture(gstream, &g);
            if (rc || e != hipSuccess || !g) {                 // capture failed: fall back to eager launches for good
                if (g) (void)hipGraphDestroy(g);
                (void)hipGetLastError();
                use_graph = false;
                return decode_eager(M, n_steps, step0, s);
            }
            hipGraphExec_t ex = nullptr;
            e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
            (void)hipGraphDestroy(g);
            if (e != hipSuccess) { use_graph = false; (void)hipGetLastError(); return decode_eager(M, n_steps, step0, s); }
            it = graphs.emplace(key, ex).first;
        }
        SA_HIP(hipEventRecord(gev_in, s));
        SA_HIP(hipStreamWaitEvent(gstream, gev_in, 0));
        SA_HIP(hipGraphLaunch(it->second, gstream));
        SA_HIP(hipEventRecord(gev_out, gstream));
        SA_HIP(hipStreamWaitEvent(s, gev_out, 0));
        return SA_OK;
    }

    // Test hook: rows [0, rows) of every (layer, kv head) run of `slot`, K and V, to device buffers [layers][kv_heads][rows][head_dim] of the
    // model's dtype.
    int copy_kv_rows(int slot, int rows, void* kdst, void* vdst, hipStream_t s) override {
        if (slot < 0 || slot >= c.max_slots || rows <= 0 || rows > c.max_kv_len || !kdst || !vdst) return SA_ERR_ARG;
        const size_t run = (size_t)c.max_kv_len * c.dec_head_dim, bytes = (size_t)rows * c.dec_head_dim * sizeof(T);
        for (int l = 0; l < c.dec_layers; ++l)
            for (int h = 0; h < c.dec_kv_heads; ++h) {
                const size_t src = (((size_t)l * c.max_slots + slot) * c.dec_kv_heads + h) * run, dst = ((size_t)l * c.dec_kv_heads + h) * bytes;
                SA_HIP(hipMemcpyAsync((char*)kdst + dst, kcache + src, bytes, hipMemcpyDeviceToDevice, s));
                SA_HIP(hipMemcpyAsync((char*)vdst + dst, vcache + src, bytes, hipMemcpyDeviceToDevice, s));
            }
        return SA_OK;
    }

    // Test hook: the product path never materialises logits (EPI_ARGMAX above), so they are recomputed here from the
    // final-norm rows of the last prefill / decode step, which are still in `dlast`, with the same GEMM main loop.
    // With token masks set these are still the UNMASKED logits: the mask lives in the greedy epilogues only.
    int copy_last_logits(float* dst, int max_rows, int* rows, hipStream_t s) override {
        const int r = std::min(max_rows, last_rows);
        *rows = r;
        if (r <= 0) return SA_OK;
        const int Hd = c.dec_hidden;
        int rc;
        if (last_heads_mx) {
            if constexpr (std::is_same<T, bf16_t>::value) {
                MxArgs a{dlast8, Hd, slast, MXG(SA_MX_LM_W), Hd, MXG(SA_MX_LM_S), last_rows, c.vocab, Hd, (long)c.max_slots, (long)c.vocab};
                a.C = logits; a.ldc = c.vocab; a.bias = W(SA_RW_LM_B);
                if ((rc = launch_gemm_mx<MX_EPI_F32>(a, s))) return rc;
            }
        } else {
            GemmArgs<T, float> a{dlast, Hd, W(SA_RW_LM_W), Hd, logits, c.vocab, W(SA_RW_LM_B), nullptr, 0, last_rows, c.vocab, Hd};
            if ((rc = launch_gemm<T, float, EPI_BIAS>(a, s))) return rc;
        }
        SA_HIP(hipMemcpyAsync(dst, logits, (size_t)r * c.vocab * sizeof(float), hipMemcpyDeviceToDevice, s));
        return SA_OK;
    }
};

}  // namespace sa
