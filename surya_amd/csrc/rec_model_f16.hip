// The recogniser in float16 (SA_DTYPE_F16): RecModel<fp16_t> and the fp16 kernels only it uses, in a translation unit of their own so that
// the second 16-bit engine compiles beside rec_model.hip instead of after it.
//
// Rounding is Ty<fp16_t> / H16<fp16_t>: round to nearest even, overflow to +-inf as torch's .half(); no loss scaling, no clamping. Split-K
// slabs, softmax, norms and RoPE tables stay fp32 as in bf16. What fp16 does not take: MXFP8 decode weights and the fp8 KV cache
// (surya_rec_set_mx_weights / surya_rec_set_kv_fp8 return SA_ERR_UNSUPPORTED, as on an fp32 engine), and decode_attn_flash_kernel -- at
// Tuning::dattn = 3 an fp16 engine runs decode_attn_flash2_kernel.
#include "rec_engine.h"
#include "rec_ops.h"

namespace sa {

// launch_decode_attn<fp16_t> (layout_model.hip) at d = 128, the recogniser's head shape: the bf16 ladder's two rungs and two-buffer rule.
template <int MAXG>
static int decode_attn_flash_f16_d128(const DecodeAttnArgs<fp16_t>& a, hipStream_t s) {
    const Tuning& t = tuning();
    if (t.dattn_db == 1 || (t.dattn_db == 0 && !t.graph && a.ctx_bound > 128 && a.rows * a.nkv <= 256))
        return decode_attn_as<decode_attn_flash2_kernel<128, MAXG, true, fp16_t>>(a, decode_attn_flash2_lds<128, MAXG, true>(), s, a.out8, a.sout, a.srows);
    return decode_attn_as<decode_attn_flash2_kernel<128, MAXG, false, fp16_t>>(a, decode_attn_flash2_lds<128, MAXG, false>(), s, a.out8, a.sout, a.srows);
}
int decode_attn_f16_d128(const DecodeAttnArgs<fp16_t>& a, hipStream_t s) {
    const int G = a.nq / a.nkv;
    if (a.d != 128 || a.out8 || G < 1 || a.nq % a.nkv) return SA_ERR_UNSUPPORTED;
    if (G <= 5) return decode_attn_flash_f16_d128<5>(a, s);
    if (G <= 8) return decode_attn_flash_f16_d128<8>(a, s);
    return SA_ERR_UNSUPPORTED;
}

// for surya_rec_create / surya_rec_workspace_bytes / surya_gemm_ring_status (rec_model.hip)
size_t rec_f16_workspace_bytes(const surya_rec_config& cfg) { return RecModel<fp16_t>::layout(cfg, nullptr); }
int rec_f16_create(const surya_rec_config& cfg, const void* const* weights, int n, std::unique_ptr<RecBase>& out) {
    auto m = std::make_unique<RecModel<fp16_t>>();
    const int rc = m->init(cfg, weights, n);
    out = std::move(m);
    return rc;
}
int rec_f16_ring_error(bool reset) { return ring_error(reset); }     // this unit's ring_error_word (gemm_ring.h)

// the fp16 arm of surya_op_lm_head_partials / surya_op_lm_head_topk (rec_model.hip): the lm_head launch of RecModel<fp16_t>::heads, masked (tm) or not
int op_lm_head_f16(const void* X, const void* W, const void* bias, int M, int N, int K, const TokenMask* tm, float4* amax, float2* alt, int* bn_used,
                   hipStream_t s, const ForcedCols* fc) {
    GemmArgs<fp16_t, float> a{(const fp16_t*)X, (long)K, (const fp16_t*)W, (long)K, nullptr, (long)N, (const fp16_t*)bias, nullptr, 0, M, N, K};
    a.amax = amax;
    int rc;
    if (fc) {                       // surya_op_lm_head_forced
        a.forced = *fc;
        rc = launch_gemm<fp16_t, float, EPI_FORCED>(a, s);
    } else if (alt) {                      // surya_op_lm_head_topk
        if (tm) a.tmask = *tm;
        a.alt = alt;
        rc = launch_gemm<fp16_t, float, EPI_TOPK>(a, s);
    } else if (tm) {
        a.tmask = *tm;
        rc = launch_gemm<fp16_t, float, EPI_ARGMAX_MASK>(a, s);
    } else {
        rc = launch_gemm<fp16_t, float, EPI_ARGMAX>(a, s);
    }
    *bn_used = a.bn_used;
    return rc;
}

// the fp16 arm of surya_op_gemm_rope (rec_model.hip): the vision qkv projection as RecModel<fp16_t>::encode launches it
int op_gemm_rope_f16(const void* X, long ldx, const void* W, long ldw, void* C, long ldc, const void* bias, const float* rope, int rope_cols,
                     int rope_D, int M, int N, int K, hipStream_t s) {
    GemmArgs<fp16_t, fp16_t> a{(const fp16_t*)X, ldx, (const fp16_t*)W, ldw, (fp16_t*)C, ldc, (const fp16_t*)bias, nullptr, 0, M, N, K};
    a.rope = reinterpret_cast<const float2*>(rope); a.rope_cols = rope_cols; a.rope_D = rope_D;
    return launch_gemm<fp16_t, fp16_t, EPI_ROPE>(a, s);
}

// the fp16 arm of the surya_op_rec_* entries (rec_model.hip): the launchers of kernels.h on the fp16 instances
int op_rec_f16(int op, const void* args, hipStream_t s) { return rec_op_any<fp16_t>(op, args, s); }

}  // namespace sa

using namespace sa;

extern "C" {

int surya_op_rec_gemm_f16(int mode, int epi, const void* X, long ldx, const void* W, long ldw, void* C, long ldc, const void* bias, const void* R,
                          long ldr, int M, int N, int K, float* amax, int* bn_used, void* stream) {
    if (!X || !W) return SA_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const fp16_t *x = (const fp16_t*)X, *w = (const fp16_t*)W, *b = (const fp16_t*)bias;
    if (mode == 0) {                                  // 16-bit output: the encoder's and the decoder's epilogues
        if (!C) return SA_ERR_ARG;
        GemmArgs<fp16_t, fp16_t> a{x, ldx, w, ldw, (fp16_t*)C, ldc, b, (const fp16_t*)R, ldr, M, N, K};
        switch (epi) {
            case EPI_BIAS: return launch_gemm<fp16_t, fp16_t, EPI_BIAS>(a, s);
            case EPI_RESIDUAL: return R ? launch_gemm<fp16_t, fp16_t, EPI_RESIDUAL>(a, s) : SA_ERR_ARG;
            case EPI_GELU: return launch_gemm<fp16_t, fp16_t, EPI_GELU>(a, s);
            case EPI_SWIGLU: return N % 2 ? SA_ERR_ARG : launch_gemm<fp16_t, fp16_t, EPI_SWIGLU>(a, s);
        }
        return SA_ERR_UNSUPPORTED;
    }
    if (mode == 1) {                                  // fp32 output (surya_rec_copy_last_logits)
        if (!C || epi != EPI_BIAS) return C ? SA_ERR_UNSUPPORTED : SA_ERR_ARG;
        GemmArgs<fp16_t, float> a{x, ldx, w, ldw, (float*)C, ldc, b, nullptr, 0, M, N, K};
        return launch_gemm<fp16_t, float, EPI_BIAS>(a, s);
    }
    if (mode == 2) {                                  // greedy partials of the lm_head (C is not written)
        if (!amax || !bn_used || epi != EPI_ARGMAX) return (amax && bn_used) ? SA_ERR_UNSUPPORTED : SA_ERR_ARG;
        GemmArgs<fp16_t, float> a{x, ldx, w, ldw, nullptr, (long)N, b, nullptr, 0, M, N, K};
        a.amax = reinterpret_cast<float4*>(amax);
        const int rc = launch_gemm<fp16_t, float, EPI_ARGMAX>(a, s);
        *bn_used = a.bn_used;
        return rc;
    }
    return SA_ERR_ARG;
}

int surya_op_gemm_splitk_f16(const void* X, long ldx, const void* W, long ldw, float* part, int M, int N, int K, int* splitk, void* stream) {
    if (!X || !W || !part || !splitk) return SA_ERR_ARG;
    GemmArgs<fp16_t, fp16_t> a{reinterpret_cast<const fp16_t*>(X), ldx, reinterpret_cast<const fp16_t*>(W), ldw, nullptr, 0, nullptr, nullptr, 0, M, N, K, 1, part};
    const int rc = launch_gemm_splitk<fp16_t>(a, (hipStream_t)stream);
    *splitk = a.splitk;
    return rc;
}

}  // extern "C"
