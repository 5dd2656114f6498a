// Kernels of the OCR-error classifier (DistilBERT, surya/ocr_error/model/encoder.py) that the shared GEMM / attention kernels do not
// cover: the embedding + LayerNorm of packed tokens, the LayerNorm, the [CLS]-query attention of the last layer, the row gather and
// the label head. Rows are PACKED: token t of the call belongs to one text, tok_pos[t] is its position inside that text.
#pragma once
#include "common.h"

namespace sa {
namespace ocr {

// word_embeddings[ids[t]] + position_embeddings[tok_pos[t]] rounded to the compute dtype (the reference adds the two T tensors,
// encoder.py:86), then LayerNorm with fp32 two-pass statistics (mean, then centred variance, as F.layer_norm). One wave per row.
// Ids outside [0, vocab) are clamped: the host checks them, the clamp keeps a bad id from reading outside the table.
template <typename T>
__global__ __launch_bounds__(256) void embed_ln_kernel(const int* __restrict__ ids, const int* __restrict__ tok_pos, const T* __restrict__ word,
                                                       const T* __restrict__ pos, const T* __restrict__ w, const T* __restrict__ b,
                                                       T* __restrict__ y, int rows, int C, int vocab, float eps) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int id = min(max(ids[row], 0), vocab - 1);
    const T* wr = word + (long)id * C;
    const T* pr = pos + (long)tok_pos[row] * C;
    float s = 0.f;
    for (int c = lane * 4; c < C; c += 256) {
        float a[4], p[4];
        load4(wr + c, a); load4(pr + c, p);
#pragma unroll
        for (int i = 0; i < 4; ++i) s += Ty<T>::rnd(a[i] + p[i]);
    }
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
    for (int c = lane * 4; c < C; c += 256) {
        float a[4], p[4];
        load4(wr + c, a); load4(pr + c, p);
#pragma unroll
        for (int i = 0; i < 4; ++i) { const float d = Ty<T>::rnd(a[i] + p[i]) - mean; q += d * d; }
    }
    const float rstd = rsqrtf(wave_sum(q) / (float)C + eps);
    T* yr = y + (long)row * C;
    for (int c = lane * 4; c < C; c += 256) {
        float a[4], p[4], wv[4], bv[4], o[4];
        load4(wr + c, a); load4(pr + c, p); load4(w + c, wv); load4(b + c, bv);
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = (Ty<T>::rnd(a[i] + p[i]) - mean) * rstd * wv[i] + bv[i];
        store4(yr + c, o[0], o[1], o[2], o[3]);
    }
}

// LayerNorm of packed rows (sa_layer_norm / output_layer_norm, encoder.py:417-420): one wave per row, fp32 two-pass statistics as in
// embed_ln_kernel. (layout_kernels.h has the same arithmetic for the Swin stages; its non-template kernels cannot enter a second TU.)
template <typename T>
__global__ __launch_bounds__(256) void layernorm_kernel(const T* __restrict__ x, const T* __restrict__ w, const T* __restrict__ b,
                                                        T* __restrict__ y, int rows, int C, float eps) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const T* xr = x + (long)row * C;
    float s = 0.f;
    for (int c = lane * 4; c < C; c += 256) {
        float v[4];
        load4(xr + c, v);
        s += v[0] + v[1] + v[2] + v[3];
    }
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
    for (int c = lane * 4; c < C; c += 256) {
        float v[4];
        load4(xr + c, v);
#pragma unroll
        for (int i = 0; i < 4; ++i) { const float d = v[i] - mean; q += d * d; }
    }
    const float rstd = rsqrtf(wave_sum(q) / (float)C + eps);
    T* yr = y + (long)row * C;
    for (int c = lane * 4; c < C; c += 256) {
        float v[4], wv[4], bv[4];
        load4(xr + c, v); load4(w + c, wv); load4(b + c, bv);
        store4(yr + c, (v[0] - mean) * rstd * wv[0] + bv[0], (v[1] - mean) * rstd * wv[1] + bv[1], (v[2] - mean) * rstd * wv[2] + bv[2],
               (v[3] - mean) * rstd * wv[3] + bv[3]);
    }
}

// out[i] = x[rows[i]] (rows of C elements, C % 4 == 0): the [CLS] rows of the packed hidden states.
template <typename T>
__global__ void gather_rows_kernel(const T* __restrict__ x, const int* __restrict__ rows, T* __restrict__ out, int n, int C) {
    const int i = blockIdx.x;
    if (i >= n) return;
    const T* src = x + (long)rows[i] * C;
    T* dst = out + (long)i * C;
    for (int c = threadIdx.x * 4; c < C; c += blockDim.x * 4) {
        float v[4];
        load4(src + c, v);
        store4(dst + c, v[0], v[1], v[2], v[3]);
    }
}

// Attention of ONE query per text -- its [CLS] row, the only row the classification head reads (encoder.py:760-761) -- over the text's
// L <= max_pos keys, every head; the 16-bit modes (T = bf16_t or fp16_t through Ty<T> / H16<T>: bf16's last layer, fp16's at
// ocrerr_cls_only = 2). One workgroup per text, shaped like a decode step: the packed qkv rows [T][3 dim] (q | k | v, head h at columns
// h * D) of the text are read once.
//   scores   item (key j, head h) per thread, fp32 dot products of the 16-bit q and k rows, kept in LDS;
//   softmax  a wave per head walks the keys in 64-key chunks with the running max of attn_mfma_kernel (the same chunk boundaries, so
//            the same max at every chunk) and rounds the un-normalised exp() values to T as that kernel rounds its P fragment (fp16:
//            entries below 2^-14 become subnormals, as there);
//            the row sum takes the unrounded values, as there; chunk c's P is later scaled by exp(m_c - m_final) / l;
//   P V      a thread per pair of output columns, keys in order, fp32 sums.
// The score and P V sums associate differently from the MFMA kernel: agreement to fp32 rounding of the 16-bit inputs, not to the bit
// (which is why fp16, whose finer steps such a difference crosses 8x as often as bf16's, takes the MFMA kernel by default).
// LDS: q [dim] + P [heads][NC * 64] + chunk factors [heads][NC] floats (dynamic; the host sizes it for max_pos).
template <typename T, int D>
__global__ __launch_bounds__(256) void cls_attn_kernel(const T* __restrict__ qkv, const int* __restrict__ starts, const int* __restrict__ lens,
                                                       T* __restrict__ out, int dim, int heads, float scale) {
    static_assert(sizeof(T) == 2, "16-bit storage types");
    extern __shared__ __attribute__((aligned(16))) float cls_sm[];
    const int t = blockIdx.x, L = lens[t], tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int NC = (L + 63) / 64, Lp = NC * 64;
    const long ld = 3L * dim;
    const T* base = qkv + (long)starts[t] * ld;
    float* qs = cls_sm;
    float* ps = qs + dim;
    float* fac = ps + (long)heads * Lp;
    for (int c = tid; c < dim; c += 256) qs[c] = Ty<T>::ld(base + c);
    __syncthreads();
    for (int it = tid; it < heads * L; it += 256) {
        const int j = it / heads, h = it - j * heads;
        const T* kr = base + (long)j * ld + dim + h * D;
        const float* qh = qs + h * D;
        float s = 0.f;
#pragma unroll
        for (int d = 0; d < D; d += 8) {
            const uint4 raw = *reinterpret_cast<const uint4*>(kr + d);
            float kv[8];
            unpack16(raw, kv, (T*)nullptr);
#pragma unroll
            for (int e = 0; e < 8; ++e) s += qh[d + e] * kv[e];
        }
        ps[h * Lp + j] = s;
    }
    __syncthreads();
    const float sl2 = scale * 1.44269504088896340736f;
    for (int h = wave; h < heads; h += 4) {
        float* ph = ps + h * Lp;
        float m = -INFINITY, l = 0.f, my_m = -INFINITY;
        for (int c = 0; c < NC; ++c) {
            const int j = c * 64 + lane;
            const float sv = j < L ? ph[j] : -INFINITY;
            const float mnew = fmaxf(m, wave_max(sv));          // finite: every chunk starts below L
            const float alpha = exp2f((m - mnew) * sl2);
            const float p = j < L ? exp2f((sv - mnew) * sl2) : 0.f;
            l = l * alpha + wave_sum(p);
            ph[j] = Ty<T>::rnd(p);
            if (lane == c) my_m = mnew;
            m = mnew;
        }
        for (int c = lane; c < NC; c += 64) {
            const float mc = c < 64 ? my_m : m;                 // (NC <= 64: max_pos <= 4096 is checked at create)
            fac[h * NC + c] = exp2f((mc - m) * sl2) / l;
        }
    }
    __syncthreads();
    const T* vb = base + 2L * dim;
    for (int o = tid * 2; o < dim; o += 512) {
        const int h = o / D;
        const float* ph = ps + h * Lp;
        float a0 = 0.f, a1 = 0.f;
        for (int c = 0; c < NC; ++c) {
            float c0 = 0.f, c1 = 0.f;
            const int j1 = min(L, c * 64 + 64);
            for (int j = c * 64; j < j1; ++j) {
                const uint32_t raw = *reinterpret_cast<const uint32_t*>(vb + (long)j * ld + o);
                const float p = ph[j];
                c0 += p * H16<T>::lo(raw);
                c1 += p * H16<T>::hi(raw);
            }
            const float f = fac[h * NC + c];
            a0 += c0 * f;
            a1 += c1 * f;
        }
        store2(out + (long)t * dim + o, a0, a1);
    }
}

// Classification head after pre_classifier + ReLU (a GEMM at M = texts): logits = pre @ classifier^T + bias, rounded to the compute
// dtype (the reference's logits are T tensors), and the first argmax (torch.argmax). One wave per text; fp32 sums in a fixed order.
template <typename T>
__global__ __launch_bounds__(64) void cls_head_kernel(const T* __restrict__ pre, const T* __restrict__ w, const T* __restrict__ b,
                                                      float* __restrict__ logits, int* __restrict__ labels, int dim, int num_labels) {
    const int t = blockIdx.x, lane = threadIdx.x;
    const T* x = pre + (long)t * dim;
    float best = -INFINITY;
    int arg = 0;
    for (int j = 0; j < num_labels; ++j) {
        const T* wr = w + (long)j * dim;
        float s = 0.f;
        for (int k = lane; k < dim; k += 64) s += Ty<T>::ld(x + k) * Ty<T>::ld(wr + k);
        const float v = Ty<T>::rnd(wave_sum(s) + Ty<T>::ld(b + j));
        if (lane == 0) logits[(long)t * num_labels + j] = v;
        if (v > best) { best = v; arg = j; }                   // strict: the first of equal maxima (NaN never wins)
    }
    if (lane == 0) labels[t] = arg;
}

// ---- launchers: the one launch of each kernel, shared by OcrErrModel and the surya_op_ocrerr_* hooks (ocr_error_model.hip)
template <typename T>
static inline int launch_embed_ln(const int* ids, const int* tok_pos, const T* word, const T* pos, const T* w, const T* b, T* y, int rows, int C,
                                  int vocab, float eps, hipStream_t s) {
    if (rows <= 0) return SA_OK;
    hipLaunchKernelGGL(embed_ln_kernel<T>, dim3(cdiv(rows, 4)), dim3(256), 0, s, ids, tok_pos, word, pos, w, b, y, rows, C, vocab, eps);
    return (int)hipGetLastError();
}

template <typename T>
static inline int launch_layernorm(const T* x, const T* w, const T* b, T* y, int rows, int C, float eps, hipStream_t s) {
    if (rows <= 0) return SA_OK;
    hipLaunchKernelGGL(layernorm_kernel<T>, dim3(cdiv(rows, 4)), dim3(256), 0, s, x, w, b, y, rows, C, eps);
    return (int)hipGetLastError();
}

template <typename T>
static inline int launch_gather_rows(const T* x, const int* rows_idx, T* out, int n, int C, hipStream_t s) {
    if (n <= 0) return SA_OK;
    hipLaunchKernelGGL(gather_rows_kernel<T>, dim3(n), dim3(64), 0, s, x, rows_idx, out, n, C);
    return (int)hipGetLastError();
}

// LDS of cls_attn_kernel for texts of up to max_len tokens: q [dim] + P [heads][NC * 64] + chunk factors [heads][NC] floats
static inline size_t cls_attn_lds_bytes(int dim, int heads, int max_len) {
    const long ncmax = (max_len + 63) / 64;
    return (size_t)(dim + (long)heads * ncmax * 64 + (long)heads * ncmax) * sizeof(float);
}

// starts / lens: device [n]; every len in 1 .. max_len (the caller checks them on the host). 16-bit storage only; head_dim D in
// {32, 64, 80, 128}, max_len <= 4096 (the kernel keeps a chunk's running max in lane `chunk`) and the LDS within 64 KB, else SA_ERR_UNSUPPORTED.
template <typename T>
static inline int launch_cls_attn(int D, const T* qkv, const int* starts, const int* lens, int n, T* out, int dim, int heads, int max_len,
                                  float scale, hipStream_t s) {
    if constexpr (sizeof(T) == 2) {
        if (n <= 0) return SA_OK;
        if (max_len < 1 || max_len > 4096) return SA_ERR_UNSUPPORTED;
        const size_t lds = cls_attn_lds_bytes(dim, heads, max_len);
        if (lds > 64 * 1024) return SA_ERR_UNSUPPORTED;
#define SA_OCR_CLS(DD) hipLaunchKernelGGL((cls_attn_kernel<T, DD>), dim3(n), dim3(256), lds, s, qkv, starts, lens, out, dim, heads, scale)
        switch (D) {
            case 32: SA_OCR_CLS(32); break;
            case 64: SA_OCR_CLS(64); break;
            case 80: SA_OCR_CLS(80); break;
            case 128: SA_OCR_CLS(128); break;
            default: return SA_ERR_UNSUPPORTED;
        }
#undef SA_OCR_CLS
        return (int)hipGetLastError();
    } else {
        return SA_ERR_UNSUPPORTED;
    }
}

template <typename T>
static inline int launch_cls_head(const T* pre, const T* w, const T* b, float* logits, int* labels, int n, int dim, int num_labels, hipStream_t s) {
    if (n <= 0) return SA_OK;
    hipLaunchKernelGGL(cls_head_kernel<T>, dim3(n), dim3(64), 0, s, pre, w, b, logits, labels, dim, num_labels);
    return (int)hipGetLastError();
}

}  // namespace ocr
}  // namespace sa
