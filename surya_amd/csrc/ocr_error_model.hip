// OCR-error classifier on MI355X: the DistilBERT sequence classifier of surya/ocr_error (model/encoder.py) behind surya_ocrerr_* of
// include/surya_amd.h. Replaces DistilBertForSequenceClassification.forward as OCRErrorPredictor calls it (ocr_error/__init__.py:19-63).
//
// Design notes (vs the PyTorch path):
//   * texts are PACKED: one forward runs over T = sum of the text lengths; no padded row is computed anywhere. The reference's padding
//     is invisible in its result (padded keys get exactly zero softmax weight, only the [CLS] row is read), so this is exact;
//   * attention is segment attention with one segment per text (attn_mfma_kernel in bf16 and fp16, attn_valu_kernel in fp32);
//   * q_lin | k_lin | v_lin run as one GEMM; the 1 / sqrt(head_dim) of encoder.py:174 is folded into the q rows at load when it is a
//     power of two (head_dim 64: bit for bit the reference's division of the rounded projection) -- in fp32 and bf16. NOT in fp16: a
//     weight below 8 x 2^-14 would turn subnormal and lose bits, so the fp16 table carries the reference's q rows and attention scales;
//   * out_lin and lin2 add the residual in the GEMM epilogue (rounded projection + residual, rounded: the reference's two T ops),
//     lin1 applies the erf GELU there; the LayerNorms are separate row kernels;
//   * the LAST layer is computed for the [CLS] rows only (Tuning::ocrerr_cls_only): its QKV GEMM still covers every token (the [CLS]
//     query attends to all keys), then attention for one query per text and out_lin, both LayerNorms and the FFN on n rows instead of T.
//     fp32 mode runs attn_valu_kernel over each text's first 64-query tile for this (the [CLS] row comes out bit-identical to the full
//     layer's), bf16 mode the one-query cls_attn_kernel. fp16 mode runs attn_mfma_kernel over the first tile, bit-identical as in fp32:
//     cls_attn_kernel<fp16_t> (ocrerr_cls_only = 2) agrees with the matrix-core kernel to fp32 rounding only, which flips the fp16
//     rounding of ~0.4 of a text's 768 attention outputs by one step, and one such flip moves a logit by up to 1.2e-3 of the largest
//      -- bf16's steps are 8x coarser and flip 8x more rarely;
//   * GEMMs over the [CLS] rows are pinned to the 64 x 64 tile, and no GEMM here splits K: every GEMM tile walks K in the same order
//     with the same MFMA, so a text's logits do not depend on how many rows its batch mates add.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/surya_amd.h"
#include "gemm.h"
#include "kernels.h"
#include "attn_mfma.h"
#include "ocr_error_kernels.h"

namespace sa {

struct OcrErrBase {
    virtual ~OcrErrBase() {}
    virtual int forward(const int32_t* ids, const int32_t* text_len, int n, float* logits, int32_t* labels, hipStream_t s) = 0;
};

static size_t oalign(size_t v) { return (v + 255) & ~(size_t)255; }

// Every GEMM of the classifier, shared by OcrErrModel and surya_op_ocrerr_gemm: C = epilogue(X W^T + bias), X rows ldx elements apart, W [N][K],
// C and R [M][N]. pinned = the [CLS]-row GEMMs: the 64 x 64 tile whatever the text count.
template <typename T, int EPI>
static int ocr_gemm(const T* X, long ldx, const T* Wt, const T* bias, T* C, const T* R, int M, int N, int K, bool pinned, hipStream_t s) {
    GemmArgs<T, T> a{X, ldx, Wt, (long)K, C, (long)N, bias, R, (long)N, M, N, K};
    if (M <= 0) return SA_OK;
    if (pinned) return launch_gemm_cfg<T, T, 64, 64, 2, 2, EPI>(a, s);     // [CLS]-row GEMMs: one path whatever the text count
    return launch_gemm<T, T, EPI>(a, s);
}

template <typename T>
struct OcrErrModel : OcrErrBase {
    surya_ocrerr_config c;
    std::vector<const T*> w;
    int D = 64;
    float attn_scale = 1.f;
    char* arena = nullptr;
    T *x, *tmp, *h1, *att, *qkv, *ffn;            // packed rows [max_tokens][...]
    T *cx, *ctmp, *ch1, *cffn, *cpre;             // [CLS] rows [max_texts][...]
    T* catt;                                      // fp32 / fp16 [CLS] attention: [max_texts][64][dim] (a text's first query tile); one-query kernel: [max_texts][dim]
    // staging: two pinned host slots mirrored on the device, one H2D copy per forward; a slot is reused only after its copy completed
    struct Slot { char* host = nullptr; char* dev = nullptr; hipEvent_t ev = nullptr; bool pending = false; };
    Slot slot[2];
    int cur = 0;
    size_t stage_cap = 0;
    size_t cls_lds = 0;

    const T* gw(int i) const { return w[i]; }
    const T* lw(int l, int i) const { return w[SA_OW_GLOBALS + l * SA_OL_COUNT + i]; }

    int init(const surya_ocrerr_config& cfg, const void* const* weights) {
        c = cfg;
        const int nw = SA_OW_GLOBALS + c.layers * SA_OL_COUNT;
        for (int i = 0; i < nw; ++i) w.push_back(reinterpret_cast<const T*>(weights[i]));
        D = c.dim / c.heads;
        attn_scale = SA_OCRERR_Q_PRESCALED(D, c.dtype) ? 1.f : 1.f / std::sqrt((float)D);
        const long Tm = c.max_tokens, Nm = c.max_texts, E = sizeof(T);
        const size_t sizes[] = {(size_t)(Tm * c.dim * E), (size_t)(Tm * c.dim * E), (size_t)(Tm * c.dim * E), (size_t)(Tm * c.dim * E),
                                (size_t)(Tm * 3 * c.dim * E), (size_t)(Tm * c.hidden * E),
                                (size_t)(Nm * c.dim * E), (size_t)(Nm * c.dim * E), (size_t)(Nm * c.dim * E), (size_t)(Nm * c.hidden * E),
                                (size_t)(Nm * c.dim * E), (size_t)(Nm * (std::is_same<T, bf16_t>::value ? 1 : 64) * c.dim * E)};
        size_t total = 0;
        for (size_t b : sizes) total += oalign(b);
        SA_HIP(hipMalloc((void**)&arena, total));
        poison_arena(arena, total);
        T** ptrs[] = {&x, &tmp, &h1, &att, &qkv, &ffn, &cx, &ctmp, &ch1, &cffn, &cpre, &catt};
        size_t off = 0;
        for (int i = 0; i < 12; ++i) { *ptrs[i] = reinterpret_cast<T*>(arena + off); off += oalign(sizes[i]); }
        // per forward: tok_pos [T], cls rows [n], text lengths [n], tiles (seg, q0) [<= T / 64 + n] x 2, offsets 4 x 2 x [n] longs
        const long tiles = Tm / 64 + Nm + 1;
        stage_cap = oalign(Tm * 4) + 2 * oalign(Nm * 4) + 4 * oalign(tiles * 4) + 8 * oalign(Nm * 8) + 4096;
        for (Slot& sl : slot) {
            SA_HIP(hipHostMalloc((void**)&sl.host, stage_cap, hipHostMallocDefault));
            SA_HIP(hipMalloc((void**)&sl.dev, stage_cap));
            SA_HIP(hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming));
        }
        cls_lds = ocr::cls_attn_lds_bytes(c.dim, c.heads, c.max_pos);
        if (sizeof(T) == 2 && cls_lds > 64 * 1024) return SA_ERR_UNSUPPORTED;
        return SA_OK;
    }
    ~OcrErrModel() override {
        for (Slot& sl : slot) {
            if (sl.pending) (void)hipEventSynchronize(sl.ev);
            if (sl.host) (void)hipHostFree(sl.host);
            if (sl.dev) (void)hipFree(sl.dev);
            if (sl.ev) (void)hipEventDestroy(sl.ev);
        }
        if (arena) (void)hipFree(arena);
    }

    template <int EPI>
    int gemm(const T* X, long ldx, const T* Wt, const T* bias, T* C, const T* R, int M, int N, int K, bool pinned, hipStream_t s) {
        return ocr_gemm<T, EPI>(X, ldx, Wt, bias, C, R, M, N, K, pinned, s);
    }
    int layernorm(const T* in, const T* wt, const T* b, T* out, int rows, hipStream_t s) {
        return ocr::launch_layernorm<T>(in, wt, b, out, rows, c.dim, c.ln_eps, s);
    }
    int attention(const T* q, T* o, const AttnSegs& sg, int n_tiles, long o_row, hipStream_t s) {
        const long ld = 3L * c.dim;
        return launch_attn<T>(D, q, q + c.dim, q + 2 * c.dim, o, sg, n_tiles, c.heads, ld, D, ld, D, o_row, D, 1, 0, attn_scale, s);
    }
    int cls_attention(const int* starts, const int* lens, int n, hipStream_t s) {
        return ocr::launch_cls_attn<T>(D, qkv, starts, lens, n, catt, c.dim, c.heads, c.max_pos, attn_scale, s);
    }

    int forward(const int32_t* ids, const int32_t* text_len, int n, float* logits, int32_t* labels, hipStream_t s) override {
        if (n <= 0) return SA_OK;
        if (n > c.max_texts) return SA_ERR_SHAPE;
        long T_ = 0;
        for (int i = 0; i < n; ++i) {
            if (text_len[i] < 1 || text_len[i] > c.max_pos) return SA_ERR_SHAPE;
            T_ += text_len[i];
        }
        if (T_ > c.max_tokens) return SA_ERR_SHAPE;
        const int Tn = (int)T_;
        // ---- host plan -> one staged copy
        Slot& sl = slot[cur];
        cur ^= 1;
        if (sl.pending) { SA_HIP(hipEventSynchronize(sl.ev)); sl.pending = false; }
        size_t off = 0;
        auto take = [&](size_t bytes) { const size_t o = off; off = oalign(off + bytes); return o; };
        const size_t o_pos = take((size_t)Tn * 4), o_start = take((size_t)n * 4), o_len = take((size_t)n * 4);
        int n_tiles = 0;
        for (int i = 0; i < n; ++i) n_tiles += cdiv(text_len[i], 64);
        const size_t o_tseg = take((size_t)n_tiles * 4), o_tq0 = take((size_t)n_tiles * 4), o_cseg = take((size_t)n * 4), o_cq0 = take((size_t)n * 4);
        const size_t o_qo = take((size_t)n * 8), o_ko = take((size_t)n * 8), o_vo = take((size_t)n * 8), o_oo = take((size_t)n * 8),
                     o_co = take((size_t)n * 8);
        if (off > stage_cap) return SA_ERR_SHAPE;
        int* h_pos = reinterpret_cast<int*>(sl.host + o_pos);
        int* h_start = reinterpret_cast<int*>(sl.host + o_start);
        int* h_len = reinterpret_cast<int*>(sl.host + o_len);
        int* h_tseg = reinterpret_cast<int*>(sl.host + o_tseg);
        int* h_tq0 = reinterpret_cast<int*>(sl.host + o_tq0);
        int* h_cseg = reinterpret_cast<int*>(sl.host + o_cseg);
        int* h_cq0 = reinterpret_cast<int*>(sl.host + o_cq0);
        long* h_qo = reinterpret_cast<long*>(sl.host + o_qo);
        long* h_ko = reinterpret_cast<long*>(sl.host + o_ko);
        long* h_vo = reinterpret_cast<long*>(sl.host + o_vo);
        long* h_oo = reinterpret_cast<long*>(sl.host + o_oo);
        long* h_co = reinterpret_cast<long*>(sl.host + o_co);
        {
            int t = 0, k = 0;
            for (int i = 0; i < n; ++i) {
                const int L = text_len[i];
                h_start[i] = t; h_len[i] = L;
                for (int p = 0; p < L; ++p) h_pos[t + p] = p;
                for (int q0 = 0; q0 < L; q0 += 64) { h_tseg[k] = i; h_tq0[k] = q0; ++k; }
                h_cseg[i] = i; h_cq0[i] = 0;
                h_qo[i] = (long)t * 3 * c.dim; h_ko[i] = h_qo[i]; h_vo[i] = h_qo[i];      // (the k / v column offsets are in the base pointers)
                h_oo[i] = (long)t * c.dim;
                h_co[i] = (long)i * 64 * c.dim;
                t += L;
            }
        }
        SA_HIP(hipMemcpyAsync(sl.dev, sl.host, off, hipMemcpyHostToDevice, s));
        SA_HIP(hipEventRecord(sl.ev, s));
        sl.pending = true;
        const int* d_pos = reinterpret_cast<const int*>(sl.dev + o_pos);
        const int* d_start = reinterpret_cast<const int*>(sl.dev + o_start);
        const int* d_len = reinterpret_cast<const int*>(sl.dev + o_len);
        AttnSegs full{reinterpret_cast<const int*>(sl.dev + o_tseg), reinterpret_cast<const int*>(sl.dev + o_tq0), d_len,
                      reinterpret_cast<const long*>(sl.dev + o_qo), reinterpret_cast<const long*>(sl.dev + o_ko),
                      reinterpret_cast<const long*>(sl.dev + o_vo), reinterpret_cast<const long*>(sl.dev + o_oo)};
        AttnSegs first = full;                       // each text's first 64-query tile, output rows [text][64][dim] in catt (fp32 [CLS] path)
        first.tile_seg = reinterpret_cast<const int*>(sl.dev + o_cseg);
        first.tile_q0 = reinterpret_cast<const int*>(sl.dev + o_cq0);
        first.o_off = reinterpret_cast<const long*>(sl.dev + o_co);

        // ---- embeddings
        int rc = ocr::launch_embed_ln<T>(ids, d_pos, gw(SA_OW_WORD), gw(SA_OW_POS), gw(SA_OW_EMB_LN_W), gw(SA_OW_EMB_LN_B), x, Tn, c.dim, c.vocab,
                                         c.ln_eps, s);
        if (rc) return rc;
        const int dim = c.dim, hid = c.hidden;
        const bool cls_only = tuning().ocrerr_cls_only != 0;
        for (int l = 0; l < c.layers; ++l) {
            const bool last_cls = cls_only && l == c.layers - 1;
            if ((rc = gemm<EPI_BIAS>(x, dim, lw(l, SA_OL_QKV_W), lw(l, SA_OL_QKV_B), qkv, nullptr, Tn, 3 * dim, dim, false, s))) return rc;
            if (!last_cls) {
                if ((rc = attention(qkv, att, full, n_tiles, dim, s))) return rc;
                if ((rc = gemm<EPI_RESIDUAL>(att, dim, lw(l, SA_OL_OUT_W), lw(l, SA_OL_OUT_B), tmp, x, Tn, dim, dim, false, s))) return rc;
                if ((rc = layernorm(tmp, lw(l, SA_OL_SA_LN_W), lw(l, SA_OL_SA_LN_B), h1, Tn, s))) return rc;
                if ((rc = gemm<EPI_GELU>(h1, dim, lw(l, SA_OL_LIN1_W), lw(l, SA_OL_LIN1_B), ffn, nullptr, Tn, hid, dim, false, s))) return rc;
                if ((rc = gemm<EPI_RESIDUAL>(ffn, hid, lw(l, SA_OL_LIN2_W), lw(l, SA_OL_LIN2_B), tmp, h1, Tn, dim, hid, false, s))) return rc;
                if ((rc = layernorm(tmp, lw(l, SA_OL_OUT_LN_W), lw(l, SA_OL_OUT_LN_B), x, Tn, s))) return rc;
                continue;
            }
            // last layer, [CLS] rows only
            long att_ld = dim;
            // the one-query kernel: bf16 always, fp16 at ocrerr_cls_only = 2 (the A/B arm); else the text's first query tile on the full layer's kernel
            const bool one_query = std::is_same<T, bf16_t>::value || (std::is_same<T, fp16_t>::value && tuning().ocrerr_cls_only == 2);
            if (!one_query) {
                if ((rc = attention(qkv, catt, first, n, dim, s))) return rc;
                att_ld = 64L * dim;                  // row 0 of each text's 64-row block
            } else {
                if ((rc = cls_attention(d_start, d_len, n, s))) return rc;
            }
            if ((rc = ocr::launch_gather_rows<T>(x, d_start, cx, n, dim, s))) return rc;
            if ((rc = gemm<EPI_RESIDUAL>(catt, att_ld, lw(l, SA_OL_OUT_W), lw(l, SA_OL_OUT_B), ctmp, cx, n, dim, dim, true, s))) return rc;
            if ((rc = layernorm(ctmp, lw(l, SA_OL_SA_LN_W), lw(l, SA_OL_SA_LN_B), ch1, n, s))) return rc;
            if ((rc = gemm<EPI_GELU>(ch1, dim, lw(l, SA_OL_LIN1_W), lw(l, SA_OL_LIN1_B), cffn, nullptr, n, hid, dim, true, s))) return rc;
            if ((rc = gemm<EPI_RESIDUAL>(cffn, hid, lw(l, SA_OL_LIN2_W), lw(l, SA_OL_LIN2_B), ctmp, ch1, n, dim, hid, true, s))) return rc;
            if ((rc = layernorm(ctmp, lw(l, SA_OL_OUT_LN_W), lw(l, SA_OL_OUT_LN_B), cx, n, s))) return rc;
        }
        if (!cls_only || c.layers == 0) {
            if ((rc = ocr::launch_gather_rows<T>(x, d_start, cx, n, dim, s))) return rc;
        }
        // ---- head: pre_classifier + ReLU (GEMM at M = n), classifier + argmax
        if ((rc = gemm<EPI_RELU>(cx, dim, gw(SA_OW_PRE_W), gw(SA_OW_PRE_B), cpre, nullptr, n, dim, dim, true, s))) return rc;
        return ocr::launch_cls_head<T>(cpre, gw(SA_OW_CLS_W), gw(SA_OW_CLS_B), logits, labels, n, dim, c.num_labels, s);
    }
};

// surya_op_gemm / surya_op_attn in fp16 (rec_model.hip): the GELU epilogue and segment attention exactly as OcrErrModel<fp16_t> launches
// them, instantiated in this translation unit beside it
int op_gemm_f16_gelu(const void* X, long ldx, const void* W, long ldw, void* C, long ldc, const void* bias, int M, int N, int K, hipStream_t s) {
    GemmArgs<fp16_t, fp16_t> a{(const fp16_t*)X, ldx, (const fp16_t*)W, ldw, (fp16_t*)C, ldc, (const fp16_t*)bias, nullptr, 0, M, N, K};
    return launch_gemm<fp16_t, fp16_t, EPI_GELU>(a, s);
}
int op_attn_f16(int D, const void* q, const void* k, const void* v, void* o, const AttnSegs& sg, int n_tiles, int heads, long q_row, long q_head,
                long k_row, long k_head, long o_row, long o_head, int group, int causal, float scale, hipStream_t s) {
    return launch_attn<fp16_t>(D, (const fp16_t*)q, (const fp16_t*)k, (const fp16_t*)v, (fp16_t*)o, sg, n_tiles, heads, q_row, q_head, k_row, k_head,
                               o_row, o_head, group, causal, scale, s);
}

// the bodies of surya_op_ocrerr_cls_attn / surya_op_ocrerr_gemm (below) per storage type
template <typename T>
static int op_cls_attn(int head_dim, const void* qkv, const int32_t* host_starts, const int32_t* host_lens, int n, void* out, int dim, int heads,
                       int max_len, float scale, hipStream_t s) {
    int* d = nullptr;                                     // starts [n] | lens [n]
    std::vector<int> h(2 * (size_t)n);
    std::copy(host_starts, host_starts + n, h.begin());
    std::copy(host_lens, host_lens + n, h.begin() + n);
    SA_HIP(hipMalloc((void**)&d, h.size() * sizeof(int)));
    int rc = (int)hipMemcpyAsync(d, h.data(), h.size() * sizeof(int), hipMemcpyHostToDevice, s);
    if (!rc) rc = ocr::launch_cls_attn<T>(head_dim, (const T*)qkv, d, d + n, n, (T*)out, dim, heads, max_len, scale, s);
    const int rs = (int)hipStreamSynchronize(s);          // the tables above are freed on return
    (void)hipFree(d);
    return rc ? rc : rs;
}

template <typename T>
static int op_ocr_gemm(int epi, int pinned, const void* X, long ldx, const void* W, const void* bias, void* C, const void* R, int M, int N, int K,
                       hipStream_t s) {
    constexpr int V = 16 / (int)sizeof(T);                // elements per 16-byte chunk: rows of X, W, C and R are read and written in them
    if (K % Ty<T>::KE || N % 4 || N % V || ldx % V || ldx < K) return SA_ERR_SHAPE;
    const T *x = (const T*)X, *w = (const T*)W, *bb = (const T*)bias, *r = (const T*)R;
    T* c = (T*)C;
    switch (epi) {
        case EPI_BIAS: return ocr_gemm<T, EPI_BIAS>(x, ldx, w, bb, c, nullptr, M, N, K, pinned != 0, s);
        case EPI_RESIDUAL: return r ? ocr_gemm<T, EPI_RESIDUAL>(x, ldx, w, bb, c, r, M, N, K, pinned != 0, s) : (int)SA_ERR_ARG;
        case EPI_GELU: return ocr_gemm<T, EPI_GELU>(x, ldx, w, bb, c, nullptr, M, N, K, pinned != 0, s);
        case EPI_RELU: return ocr_gemm<T, EPI_RELU>(x, ldx, w, bb, c, nullptr, M, N, K, pinned != 0, s);
        default: return SA_ERR_UNSUPPORTED;
    }
}

}  // namespace sa

using namespace sa;

struct surya_ocrerr { std::unique_ptr<OcrErrBase> impl; };

extern "C" {

int surya_ocrerr_create(const surya_ocrerr_config* cfg, const void* const* weights, int n_weights, surya_ocrerr** out) {
    if (!cfg || !weights || !out) return SA_ERR_ARG;
    if (cfg->dtype != SA_DTYPE_F32 && cfg->dtype != SA_DTYPE_BF16 && cfg->dtype != SA_DTYPE_F16) return SA_ERR_UNSUPPORTED;
    if (cfg->layers < 1 || cfg->heads < 1 || cfg->dim % cfg->heads || cfg->num_labels < 1 || cfg->vocab < 1) return SA_ERR_ARG;
    const int D = cfg->dim / cfg->heads;
    if (D != 32 && D != 64 && D != 80 && D != 128) return SA_ERR_UNSUPPORTED;
    if (cfg->dim % 64 || cfg->hidden % 64) return SA_ERR_SHAPE;          // GEMM K chunks (64 bf16 / fp16 or 32 fp32 elements), 16-byte rows
    if (cfg->max_pos < 1 || cfg->max_pos > 4096) return SA_ERR_UNSUPPORTED;
    if (cfg->max_texts < 1 || cfg->max_tokens < 1) return SA_ERR_ARG;
    if (n_weights != SA_OW_GLOBALS + cfg->layers * SA_OL_COUNT) return SA_ERR_ARG;
    for (int i = 0; i < n_weights; ++i)
        if (!weights[i]) return SA_ERR_ARG;
    auto* h = new surya_ocrerr();
    int rc;
    if (cfg->dtype == SA_DTYPE_F32) {
        auto* m = new OcrErrModel<float>();
        h->impl.reset(m);
        rc = m->init(*cfg, weights);
    } else if (cfg->dtype == SA_DTYPE_F16) {
        auto* m = new OcrErrModel<fp16_t>();
        h->impl.reset(m);
        rc = m->init(*cfg, weights);
    } else {
        auto* m = new OcrErrModel<bf16_t>();
        h->impl.reset(m);
        rc = m->init(*cfg, weights);
    }
    if (rc) { delete h; return rc; }
    *out = h;
    return SA_OK;
}

int surya_ocrerr_destroy(surya_ocrerr* h) {
    delete h;
    return SA_OK;
}

int surya_ocrerr_forward(surya_ocrerr* h, const int32_t* ids, const int32_t* text_len, int n_texts, float* logits, int32_t* labels,
                         void* stream) {
    if (!h || !h->impl || (n_texts > 0 && (!ids || !text_len || !logits || !labels)) || n_texts < 0) return SA_ERR_ARG;
    return h->impl->forward(ids, text_len, n_texts, logits, labels, (hipStream_t)stream);
}

// ---- the classifier's kernels alone (tests): the launchers of ocr_error_kernels.h and ocr_gemm, as OcrErrModel calls them
#define SA_OCR_BY_DTYPE(CALL)                                                \
    switch (dtype) {                                                         \
        case SA_DTYPE_F32: { typedef float T; return CALL; }                 \
        case SA_DTYPE_BF16: { typedef bf16_t T; return CALL; }               \
        case SA_DTYPE_F16: { typedef fp16_t T; return CALL; }                \
        default: return SA_ERR_UNSUPPORTED;                                  \
    }

int surya_op_ocrerr_embed_ln(int dtype, const int32_t* ids, const int32_t* tok_pos, const void* word, const void* pos, const void* w, const void* b,
                             void* y, int rows, int C, int vocab, float eps, void* stream) {
    if (!ids || !tok_pos || !word || !pos || !w || !b || !y || rows <= 0 || C <= 0 || vocab <= 0) return SA_ERR_ARG;
    if (C % 4) return SA_ERR_SHAPE;
    SA_OCR_BY_DTYPE(ocr::launch_embed_ln<T>(ids, tok_pos, (const T*)word, (const T*)pos, (const T*)w, (const T*)b, (T*)y, rows, C, vocab, eps,
                                            (hipStream_t)stream))
}

int surya_op_ocrerr_layernorm(int dtype, const void* x, const void* w, const void* b, void* y, int rows, int C, float eps, void* stream) {
    if (!x || !w || !b || !y || rows <= 0 || C <= 0) return SA_ERR_ARG;
    if (C % 4) return SA_ERR_SHAPE;
    SA_OCR_BY_DTYPE(ocr::launch_layernorm<T>((const T*)x, (const T*)w, (const T*)b, (T*)y, rows, C, eps, (hipStream_t)stream))
}

int surya_op_ocrerr_gather_rows(int dtype, const void* x, const int32_t* rows_idx, void* out, int n, int C, void* stream) {
    if (!x || !rows_idx || !out || n <= 0 || C <= 0) return SA_ERR_ARG;
    if (C % 4) return SA_ERR_SHAPE;
    SA_OCR_BY_DTYPE(ocr::launch_gather_rows<T>((const T*)x, rows_idx, (T*)out, n, C, (hipStream_t)stream))
}

int surya_op_ocrerr_cls_attn(int dtype, int head_dim, const void* qkv, const int32_t* host_starts, const int32_t* host_lens, int n, void* out,
                             int dim, int heads, int max_len, float scale, void* stream) {
    if (!qkv || !host_starts || !host_lens || !out || n <= 0 || dim <= 0 || heads <= 0 || head_dim <= 0 || max_len <= 0) return SA_ERR_ARG;
    if (dtype == SA_DTYPE_F32) return SA_ERR_UNSUPPORTED;                       // cls_attn_kernel has 16-bit storage only
    if (dtype != SA_DTYPE_BF16 && dtype != SA_DTYPE_F16) return SA_ERR_UNSUPPORTED;
    if (head_dim % 8 || dim != heads * head_dim) return SA_ERR_SHAPE;
    if (head_dim != 32 && head_dim != 64 && head_dim != 80 && head_dim != 128) return SA_ERR_UNSUPPORTED;
    if (max_len > 4096 || ocr::cls_attn_lds_bytes(dim, heads, max_len) > 64 * 1024) return SA_ERR_UNSUPPORTED;
    for (int i = 0; i < n; ++i)
        if (host_starts[i] < 0 || host_lens[i] < 1 || host_lens[i] > max_len) return SA_ERR_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == SA_DTYPE_BF16) return op_cls_attn<bf16_t>(head_dim, qkv, host_starts, host_lens, n, out, dim, heads, max_len, scale, s);
    return op_cls_attn<fp16_t>(head_dim, qkv, host_starts, host_lens, n, out, dim, heads, max_len, scale, s);
}

int surya_op_ocrerr_cls_head(int dtype, const void* pre, const void* w, const void* b, float* logits, int32_t* labels, int n, int dim,
                             int num_labels, void* stream) {
    if (!pre || !w || !b || !logits || !labels || n <= 0 || dim <= 0 || num_labels <= 0) return SA_ERR_ARG;
    SA_OCR_BY_DTYPE(ocr::launch_cls_head<T>((const T*)pre, (const T*)w, (const T*)b, logits, labels, n, dim, num_labels, (hipStream_t)stream))
}

int surya_op_ocrerr_gemm(int dtype, int epi, int pinned, const void* X, long ldx, const void* W, const void* bias, void* C, const void* R, int M,
                         int N, int K, void* stream) {
    if (!X || !W || !bias || !C || M <= 0 || N <= 0 || K <= 0 || ldx <= 0) return SA_ERR_ARG;
    SA_OCR_BY_DTYPE(op_ocr_gemm<T>(epi, pinned, X, ldx, W, bias, C, R, M, N, K, (hipStream_t)stream))
}
#undef SA_OCR_BY_DTYPE

}  // extern "C"
