// Layout model family on MI355X: Donut-Swin window-attention encoder + ADETR decoder with cross- and
// self-attention, behind surya_layout_* of include/surya_amd.h. Replaces DonutSwinLayoutModel.forward
// (surya/layout/model/encoder.py:36-80, surya/common/donut/encoder.py) and SuryaLayoutDecoder.forward
// (surya/layout/model/decoder.py:96-131, surya/common/adetr/decoder.py) as LayoutPredictor calls them
// (surya/layout/__init__.py:95-131).
//
// Design notes (vs the PyTorch path):
//   * window partition, cyclic shift and their inverses are ONE permutation table per (stage, shift): LayerNorm writes its rows
//     straight into window order, the projection output is added back through the same table -- no roll / view / permute passes;
//   * the shift mask is computed from the window's position (only the last window row / column is cut), the relative position
//     bias is gathered once at load time into [head][64][64];
//   * cross-attention K / V of the encoder states are projected once per batch in `encode` (the reference caches them at the
//     first decoder call); the decode step's self-attention reuses the recogniser's fused split-K-combine + RoPE + KV-append +
//     attention kernel (decode_attn.h) on a [layer][image][kv_head][max_boxes][d] cache;
//   * every dense layer runs on gemm.h's MFMA tiles (patch embedding = GEMM over patch rows, merge reduction, GeGLU MLP).
#include <algorithm>
#include <cstring>
#include <map>
#include <memory>
#include <set>
#include <vector>

#include "../../include/surya_amd.h"
#include "gemm.h"
#include "kernels.h"
#include "decode_attn.h"
#include "layout_kernels.h"
#include "layout_prep.h"

namespace sa {

struct LayoutBase {
    virtual ~LayoutBase() {}
    virtual int encode(const float* pixels, int B, hipStream_t s) = 0;
    virtual int decode_step(const int32_t* boxes, int B, int pos, float* cls, float* box, hipStream_t s) = 0;
    virtual int encoder_states(void* out, int B, hipStream_t s) = 0;
    virtual int select(const int32_t* src, int n) = 0;
    virtual int prefill(const int32_t* boxes, int B, int Tn, float* cls, float* box, hipStream_t s) = 0;
    virtual int set_feedback(const surya_layout_feedback* fb, int B, hipStream_t s) = 0;
    virtual int decode_steps(const int32_t* boxes, int B, int pos0, int n_steps, int ring, hipStream_t s) = 0;
    virtual int wait_steps(int ring, int B, int n_steps, float* cls, float* box, int32_t* tok) = 0;
};

static size_t lalign(size_t v) { return (v + 255) & ~(size_t)255; }

__global__ void fill_int_kernel(int* p, int v, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}


// ---------------------------------------------------------------------------------------------------------------------
// Launch code of the family's own kernels: grid, block and LDS arithmetic and the choice between the fp32 and the bf16 kernel live HERE
// only. LayoutModel and the op-level entry points (surya_op_lay_*, the end of this file) both call these, so a kernel tested alone is
// launched exactly as the engine launches it.
namespace lay {

// Window-order row of every token of an h x w grid (window_partition after F.pad to whole windows and torch.roll(-shift),
// donut/encoder.py:588-636) and the window-order rows nothing maps to (the zero padding). A grid whose smaller side does not exceed the
// window is not shifted (:551-559). Host only.
inline int window_tables(int h, int w, int ws, int shift_req, std::vector<int>& perm, std::vector<int>& pads, int& hp, int& wp, int& shift) {
    if (h <= 0 || w <= 0 || ws <= 0 || shift_req < 0 || shift_req >= ws) return SA_ERR_ARG;
    if (std::min(h, w) < ws) return SA_ERR_UNSUPPORTED;       // a map below the window: the reference's [64][64] bias would not fit either
    shift = std::min(h, w) > ws ? shift_req : 0;
    hp = (h + ws - 1) / ws * ws; wp = (w + ws - 1) / ws * ws;
    perm.assign((size_t)h * w, 0);
    std::vector<char> hit((size_t)hp * wp, 0);
    for (int y = 0; y < h; ++y)
        for (int xx = 0; xx < w; ++xx) {
            const int ys = ((y - shift) % hp + hp) % hp, xs = ((xx - shift) % wp + wp) % wp;
            const int r = ((ys / ws) * (wp / ws) + xs / ws) * ws * ws + (ys % ws) * ws + xs % ws;
            perm[(size_t)y * w + xx] = r;
            hit[r] = 1;
        }
    pads.clear();
    for (int r = 0; r < hp * wp; ++r)
        if (!hit[r]) pads.push_back(r);
    return SA_OK;
}

template <typename T>
int launch_patchify(const float* px, T* rows, int B, int C, int H, int W, int P, int Kpad, hipStream_t s) {
    const long total = (long)B * (H / P) * (W / P) * Kpad;
    hipLaunchKernelGGL(patchify_kernel<T>, dim3((unsigned)cdivl(total, 256)), dim3(256), 0, s, px, rows, B, C, H, W, P, Kpad);
    return (int)hipGetLastError();
}
template <typename T>
int launch_add_rows(T* x, const T* tab, long rows, int rpi, int C, hipStream_t s) {
    const long n4 = rows * (C / 4);
    hipLaunchKernelGGL(add_rows_kernel<T>, dim3((unsigned)cdivl(n4, 256)), dim3(256), 0, s, x, tab, rows, rpi, C);
    return (int)hipGetLastError();
}
template <typename T>
int launch_zero_rows(T* y, const int* pad_rows, int n_pad, int B, int rpi, int C, hipStream_t s) {
    const long n4 = (long)B * n_pad * (C / 4);
    hipLaunchKernelGGL(zero_rows_kernel<T>, dim3((unsigned)cdivl(n4, 256)), dim3(256), 0, s, y, pad_rows, n_pad, B, rpi, C);
    return (int)hipGetLastError();
}
template <typename T>
int launch_gather_add(T* x, const T* a, const int* pm, long rows, int rpi, int C, int rpi_src, hipStream_t s) {
    const long n4 = rows * (C / 4);
    hipLaunchKernelGGL(gather_add_kernel<T>, dim3((unsigned)cdivl(n4, 256)), dim3(256), 0, s, x, a, pm, rows, rpi, C, rpi_src);
    return (int)hipGetLastError();
}

// bf16 / fp16 rows of 128 / 256 / 512 / 1024 channels are held in registers by C / 8 lanes (layernorm_rows_bf16_kernel; 16-byte aligned rows)
// unless sa::Tuning lay_ln is 0; everything else takes the one-wave-per-row kernel.
template <typename T>
int launch_layernorm(const T* in, const T* w, const T* b, T* out, const int* pm, long rows, int rpi, int C, float eps, int rpi_out, hipStream_t s) {
    if constexpr (sizeof(T) == 2) {                                  // a 16-bit storage type
        if (rows > 0 && tuning().lay_ln) {
#define SA_LN_ROWS(LPR, NV)                                                                                                              \
    {                                                                                                                                    \
        hipLaunchKernelGGL((layernorm_rows_bf16_kernel<T, LPR, NV>), dim3((unsigned)cdivl(rows, 256 / LPR)), dim3(256), 0, s, in, w, b, out, \
                           pm, rows, rpi, eps, rpi_out);                                                                                 \
        return (int)hipGetLastError();                                                                                                   \
    }
            if (C == 128) SA_LN_ROWS(16, 1)
            if (C == 256) SA_LN_ROWS(32, 1)
            if (C == 512) SA_LN_ROWS(64, 1)
            if (C == 1024) SA_LN_ROWS(64, 2)
#undef SA_LN_ROWS
        }
    }
    hipLaunchKernelGGL(layernorm_kernel<T>, dim3((unsigned)cdivl(rows, 4)), dim3(256), 0, s, in, w, b, out, pm, rows, rpi, C, eps, rpi_out);
    return (int)hipGetLastError();
}

// one workgroup per (window of 64 tokens, head); bf16 and fp16 on the matrix cores, fp32 on the VALU
template <typename T>
int launch_window_attn(const T* qkv, const float* bias, T* out, long windows, int nh, int nkv, int nwx, int nwy, int shift, int ws, hipStream_t s) {
    if constexpr (sizeof(T) == 2)
        hipLaunchKernelGGL(swin_window_attn_mfma_kernel<T>, dim3((unsigned)windows, nh), dim3(128), 0, s, qkv, bias, out, nh, nkv, nwx, nwy, shift, ws);
    else
        hipLaunchKernelGGL(swin_window_attn_kernel<T>, dim3((unsigned)windows, nh), dim3(256), 0, s, qkv, bias, out, nh, nkv, nwx, nwy, shift, ws);
    return (int)hipGetLastError();
}

template <typename T>
int launch_merge_ln(const T* x, const T* w, const T* b, T* y, int B, int H, int W, int C, float eps, hipStream_t s) {
    const long orows = (long)B * (H / 2) * (W / 2);
    hipLaunchKernelGGL(merge_ln_kernel<T>, dim3((unsigned)cdivl(orows, 4)), dim3(256), 0, s, x, w, b, y, B, H, W, C, eps);
    return (int)hipGetLastError();
}

template <typename T>
int launch_rmsnorm(const T* x, const T* w, T* y, int rows, int C, float eps, hipStream_t s) {
    hipLaunchKernelGGL(adetr_rmsnorm_kernel<T>, dim3(cdiv(rows, 4)), dim3(256), 0, s, x, w, y, rows, C, eps);
    return (int)hipGetLastError();
}

// Cross attention over Lk cached keys. fp32: `ranges` key ranges of `chunk` keys (>= 128 keys per range, at most 8 ranges), one record of
// head_dim + 2 floats per (row, head, range) in `scratch`. bf16 / fp16: the values transposed once per encode into rows of Lkp keys (whole 32-key steps).
struct CrossPlan { int chunk, ranges, Lkp; };
inline CrossPlan cross_plan(int Lk) {
    const int n = std::max(1, std::min(8, Lk / 128));
    CrossPlan p;
    p.chunk = (Lk + n - 1) / n;
    p.ranges = (Lk + p.chunk - 1) / p.chunk;
    p.Lkp = (Lk + 31) & ~31;
    return p;
}
template <typename T>
int launch_transpose_cross_v(const T* kv, T* vT, int images, int Lk, int nkv, int d, hipStream_t s) {
    hipLaunchKernelGGL(transpose_cross_v_kernel<T>, dim3(64, images), dim3(256), 0, s, kv, vT, Lk, cross_plan(Lk).Lkp, nkv, d);
    return (int)hipGetLastError();
}
// rows query rows (S == 0: qpart is a plain [M][nq * d] matrix of T; else the sum of S <= 8 fp32 slabs [S][M][nq * d]); bf16 / fp16 read kv and vT and
// needs no scratch, fp32 reads kv and goes through scratch.
template <typename T>
int launch_cross_attn(const float* qpart, int S, int M, const T* kv, const T* vT, float* scratch, T* out, const int* item_map, int rows, int nq,
                      int nkv, int d, int Lk, float scale, hipStream_t s) {
    const int G = nq / nkv;
    if (G < 1 || G > 8 || nq % nkv || (d != 64 && d != 32) || S < 0 || S > 8 || Lk < 1) return SA_ERR_UNSUPPORTED;
    const CrossPlan cp = cross_plan(Lk);
    if constexpr (sizeof(T) == 2) {                                  // bf16 / fp16: matrix-core kernel on the transposed values (layout_kernels.h)
        if (d == 64) hipLaunchKernelGGL((cross_attn_mfma_kernel<T, 64>), dim3(rows, nkv), dim3(512), 0, s, qpart, S, M, kv, vT, out, item_map, nq, nkv, Lk,
                                        cp.Lkp, scale);
        else hipLaunchKernelGGL((cross_attn_mfma_kernel<T, 32>), dim3(rows, nkv), dim3(512), 0, s, qpart, S, M, kv, vT, out, item_map, nq, nkv, Lk, cp.Lkp,
                                scale);
    } else {
        const size_t lds = ((size_t)G * cp.chunk + (size_t)G * d + 1024) * sizeof(float);
        if (lds > 64 * 1024 - 512) return SA_ERR_UNSUPPORTED;
        dim3 grid(rows, nkv, cp.ranges);
        const int mblocks = cdiv(rows * nq * (d / 4), 256);
        if (d == 64) {
            hipLaunchKernelGGL((cross_attn_split_kernel<T, 64>), grid, dim3(256), lds, s, qpart, S, M, kv, scratch, item_map, nq, nkv, Lk, cp.chunk, scale);
            hipLaunchKernelGGL((cross_attn_merge_kernel<T, 64>), dim3(mblocks), dim3(256), 0, s, scratch, out, rows * nq, cp.ranges);
        } else {
            hipLaunchKernelGGL((cross_attn_split_kernel<T, 32>), grid, dim3(256), lds, s, qpart, S, M, kv, scratch, item_map, nq, nkv, Lk, cp.chunk, scale);
            hipLaunchKernelGGL((cross_attn_merge_kernel<T, 32>), dim3(mblocks), dim3(256), 0, s, scratch, out, rows * nq, cp.ranges);
        }
    }
    return (int)hipGetLastError();
}

// one workgroup per row, one 4-channel chunk per thread, whole waves
template <typename T>
int launch_reduce_norm(const float* part, int S, int M, const T* res, const T* bias, T* xo, const T* nw, T* y, int H, float eps, hipStream_t s) {
    if (H % 4 || H < 4 || H > 4096 || S < 1 || S > 8) return SA_ERR_UNSUPPORTED;
    const int threads = std::min(1024, ((H / 4 + 63) / 64) * 64);
    hipLaunchKernelGGL(splitk_residual_adetr_norm_kernel<T>, dim3(M), dim3(threads), 0, s, part, S, M, res, bias, xo, nw, y, H, eps);
    return (int)hipGetLastError();
}

// one workgroup per (row, kv head); the prompt's rotated keys and its values sit in LDS as fp32
template <typename T>
int launch_prefill_attn(const T* qkv, T* out, T* kc, T* vc, const float2* rope_cs, int B, int Tn, int nq, int nkv, int d, int Tmax, float scale,
                        hipStream_t s) {
    if ((d != 64 && d != 32) || nq % nkv || Tn < 1 || Tn > Tmax) return SA_ERR_UNSUPPORTED;
    const size_t lds = (size_t)2 * Tn * d * sizeof(float);
    if (lds > 64 * 1024 - 512) return SA_ERR_UNSUPPORTED;
    if (d == 64) hipLaunchKernelGGL((adetr_prefill_attn_kernel<T, 64>), dim3(B, nkv), dim3(256), lds, s, qkv, out, kc, vc, rope_cs, Tn, nq, nkv, Tmax, scale);
    else hipLaunchKernelGGL((adetr_prefill_attn_kernel<T, 32>), dim3(B, nkv), dim3(256), lds, s, qkv, out, kc, vc, rope_cs, Tn, nq, nkv, Tmax, scale);
    return (int)hipGetLastError();
}

// one workgroup per token row; tabs = 17 device pointers (layout: 14 box tables + label; table recognition: + category, merge, colspan)
template <typename T>
int launch_embed(int family, const int* tokens, const T* const* tabs, T* x, int rows, int Hd, int box_embed, int bbox_size, int vocab, int label_count,
                 int category_count, int merge_count, hipStream_t s) {
    if (family == SA_FAMILY_TABLE)
        hipLaunchKernelGGL(table_embed_kernel<T>, dim3(rows), dim3(256), 0, s, tokens, tabs, x, Hd, box_embed, bbox_size, vocab, category_count, merge_count);
    else
        hipLaunchKernelGGL(box_embed_kernel<T>, dim3(rows), dim3(256), 0, s, tokens, tabs, x, Hd, bbox_size, vocab, label_count);
    return (int)hipGetLastError();
}

// the heads without the fed-back token (layout_heads_kernel<T, false>): one workgroup per row, the row in LDS as fp32
template <typename T>
int launch_heads(const T* x, long ldx, const T* fnorm_w, const T* ln_w, const T* ln_b, const T* lm_w, const T* bb_w, const T* bb_b, float* cls,
                 float* box, int B, int Hd, int label_count, float rms_eps, float ln_eps, hipStream_t s) {
    if (Hd % 4 || (size_t)Hd * 4 > 64 * 1024 - 512) return SA_ERR_UNSUPPORTED;
    hipLaunchKernelGGL((layout_heads_kernel<T, false>), dim3(B), dim3(256), (size_t)Hd * 4, s, x, fnorm_w, ln_w, ln_b, lm_w, bb_w, bb_b, cls, box, Hd,
                       label_count, rms_eps, ln_eps, ldx);
    return (int)hipGetLastError();
}

}  // namespace lay

template <typename T>
struct LayoutModel : LayoutBase {
    surya_layout_config c;
    std::vector<const void*> w;
    std::vector<int> stage_base;                 // weight-table index of each stage's first entry
    int dec_base = 0;
    char* arena = nullptr;
    // encoder workspaces
    T *patch_rows, *x, *hbuf, *qkv, *att, *mlp;
    std::vector<int*> perm;                      // [stage * 2 + (shift > 0)] device permutation tables (token -> window-order row)
    std::vector<int*> pad_rows;                  // [stage * 2 + (shift > 0)] window-order rows of the zero padding (grids that are not whole windows)
    std::vector<int> pad_count;
    std::vector<int> grid_hp, grid_wp;           // per stage: the grid rounded up to whole windows
    // decoder
    T *ckv;                                      // [layer][B][Lk][2 * kvd]
    T *cvT = nullptr;                            // bf16 / fp16: [layer][B][nkv][hd][Lkp] transposed cross-attention values (cross_attn_mfma_kernel)
    int Lkp = 0;
    T *kcache, *vcache;                          // [layer][B][nkv][Tmax][hd]
    T *dx, *dh, *dq, *dattn, *dres, *dmlp;
    float* part;
    float* cross_scratch;                        // [B][nq][ranges][hd + 2] partial cross-attention records
    static constexpr int MAX_PROMPT = 64;        // tokens of a decoder prompt that prefill() takes in one pass
    size_t enc_mlp_bytes = 0, enc_qkv_bytes = 0; // sizes of the encoder workspaces prefill() borrows between two encodes
    int cross_ranges = 1;                        // key ranges of the fp32 cross attention (lay::cross_plan): sizes its scratch
    int* cross_map_dev = nullptr;                // [max_batch] decoder row -> encoded image whose K / V it cross-attends
    int batch_active = 0;                        // decoder rows of the current decode (encode: = batch; select: any re-batching)
    float2* rope_cs;
    int *boxes_dev, *slots_dev, *len_dev;
    float *cls_dev, *box_dev;
    const T** tabs_dev = nullptr;                // 17 embedding table pointers
    int tokw() const { return c.family == SA_FAMILY_TABLE ? 10 : 7; }
    char* pinned = nullptr;
    int Lk = 0, enc_rows_final = 0, batch_encoded = 0;

    const T* W(int i) const { return reinterpret_cast<const T*>(w[i]); }
    int gh() const { return c.img_h / c.patch; }
    int gw() const { return c.img_w / c.patch; }
    int kvd() const { return c.dec_kv_heads * (c.dec_hidden / c.dec_heads); }
    int hd() const { return c.dec_hidden / c.dec_heads; }

    int init(const surya_layout_config& cfg, const void* const* weights, int n) {
        c = cfg;
        w.assign(weights, weights + n);
        int idx = SA_LW_GLOBALS;
        for (int s = 0; s < c.n_stages; ++s) { stage_base.push_back(idx); idx += SA_LS_COUNT + c.depths[s] * SA_LB_COUNT; }
        dec_base = idx;
        if (n != dec_base + c.dec_layers * SA_LD_COUNT) return SA_ERR_ARG;
        const size_t B = c.max_batch, rows0 = B * gh() * gw(), E = c.embed_dim;
        int fh = gh(), fw = gw();
        for (int s = 1; s < c.n_stages; ++s) { fh /= 2; fw /= 2; }
        Lk = fh * fw;
        if (Lk > c.encoder_length) return SA_ERR_SHAPE;
        const size_t He = E << (c.n_stages - 1), Hd = c.dec_hidden, I = c.dec_inter, qd = Hd, kv = kvd();
        const size_t qkv_d = qd + 2 * kv;
        size_t off = 0;
        auto take = [&](size_t bytes) { size_t o = off; off = lalign(off + bytes); return o; };
        // window-order workspaces hold the PADDED grid of a stage (rows of whole windows); rows x width shrinks by two per stage unless the
        // padding outgrows it, so take the largest stage
        size_t win_elems = 0;
        {
            size_t h2 = gh(), w2 = gw(), dim2 = E;
            for (int s = 0; s < c.n_stages; ++s) {
                const size_t hp = (h2 + c.window - 1) / c.window * c.window, wp = (w2 + c.window - 1) / c.window * c.window;
                win_elems = std::max(win_elems, B * hp * wp * dim2);
                h2 = (h2 + 1) / 2; w2 = (w2 + 1) / 2; dim2 *= 2;
            }
        }
        const size_t o_patch = take(rows0 * 64 * sizeof(T)), o_x = take(rows0 * E * sizeof(T)), o_h = take(win_elems * sizeof(T));
        const size_t o_qkv = take(win_elems * 3 * sizeof(T)), o_att = take(win_elems * sizeof(T)), o_mlp = take(rows0 * 4 * E * sizeof(T));
        enc_qkv_bytes = win_elems * 3 * sizeof(T); enc_mlp_bytes = rows0 * 4 * E * sizeof(T);
        const size_t o_ckv = take((size_t)c.dec_layers * B * Lk * 2 * kv * sizeof(T));
        Lkp = lay::cross_plan(Lk).Lkp;
        const size_t o_cvt = take((size_t)c.dec_layers * B * kv * Lkp * sizeof(T));
        const size_t kv_elems = (size_t)c.dec_layers * B * c.dec_kv_heads * c.max_boxes * hd();
        const size_t o_k = take(kv_elems * sizeof(T)), o_v = take(kv_elems * sizeof(T));
        const size_t o_dx = take(B * Hd * sizeof(T)), o_dh = take(B * Hd * sizeof(T)), o_dq = take(B * qd * sizeof(T));
        const size_t o_da = take(B * qd * sizeof(T)), o_dr = take(B * Hd * sizeof(T)), o_dm = take(B * I * sizeof(T));
        const size_t o_part = take((size_t)8 * B * std::max(qkv_d, Hd) * sizeof(float));
        const size_t o_rope = take((size_t)c.max_boxes * (hd() / 2) * sizeof(float2));
        cross_ranges = lay::cross_plan(Lk).ranges;                   // >= 128 keys per range
        const size_t o_cscr = take(B * c.dec_heads * cross_ranges * (hd() + 2) * sizeof(float)), o_cmap = take(B * sizeof(int));
        const size_t o_boxes = take(B * 10 * sizeof(int)), o_slots = take(B * sizeof(int)), o_len = take(B * sizeof(int));
        const size_t o_cls = take(B * c.label_count * sizeof(float)), o_box = take(B * 6 * sizeof(float));
        const size_t o_tabs = take(17 * sizeof(void*));
        // permutation tables: two per stage
        std::vector<size_t> o_perm;
        {
            int h = gh(), wd = gw();
            for (int s = 0; s < c.n_stages; ++s) {
                o_perm.push_back(take((size_t)h * wd * sizeof(int)));
                o_perm.push_back(take((size_t)h * wd * sizeof(int)));
                h /= 2; wd /= 2;
            }
        }
        SA_HIP(hipMalloc((void**)&arena, off));
        poison_arena(arena, off);
        // The self-attention caches must hold FINITE data from the start: the first decode step of a row (no cached token yet) loads
        // cache row 0 as the clamped duplicate behind its masked key columns, P = 0 there, and 0 x NaN = NaN. hipMalloc does not clear
        // memory -- on a box whose last tenant left NaN bit patterns in HBM every output of that model was NaN (gpurun r04f: three tests
        // failed on one box only; SURYA_AMD_POISON=1 reproduces it everywhere). Rows only ever get overwritten with finite values.
        SA_HIP(hipMemset(arena + o_k, 0, kv_elems * sizeof(T)));
        SA_HIP(hipMemset(arena + o_v, 0, kv_elems * sizeof(T)));
        char* b = arena;
        patch_rows = (T*)(b + o_patch); x = (T*)(b + o_x); hbuf = (T*)(b + o_h); qkv = (T*)(b + o_qkv); att = (T*)(b + o_att); mlp = (T*)(b + o_mlp);
        ckv = (T*)(b + o_ckv); cvT = (T*)(b + o_cvt); kcache = (T*)(b + o_k); vcache = (T*)(b + o_v);
        dx = (T*)(b + o_dx); dh = (T*)(b + o_dh); dq = (T*)(b + o_dq); dattn = (T*)(b + o_da); dres = (T*)(b + o_dr); dmlp = (T*)(b + o_dm);
        part = (float*)(b + o_part); rope_cs = (float2*)(b + o_rope);
        cross_scratch = (float*)(b + o_cscr); cross_map_dev = (int*)(b + o_cmap);
        boxes_dev = (int*)(b + o_boxes); slots_dev = (int*)(b + o_slots); len_dev = (int*)(b + o_len);
        cls_dev = (float*)(b + o_cls); box_dev = (float*)(b + o_box); tabs_dev = (const T**)(b + o_tabs);
        {   // window-order row of every token, per stage and shift, and the window-order rows nothing maps to (lay::window_tables)
            int h = gh(), wd = gw();
            for (int s = 0; s < c.n_stages; ++s) {
                const int ws = c.window;
                if ((h % 2 || wd % 2) && s + 1 < c.n_stages) return SA_ERR_SHAPE;      // (the reference's sin-cos table is sized for grid >> stage)
                for (int sh = 0; sh < 2; ++sh) {
                    std::vector<int> p, pads;
                    int hp = 0, wp = 0, shift = 0;
                    const int trc = lay::window_tables(h, wd, ws, sh ? ws / 2 : 0, p, pads, hp, wp, shift);
                    if (trc) return trc;
                    if (!sh) { grid_hp.push_back(hp); grid_wp.push_back(wp); }
                    int* d = (int*)(b + o_perm[2 * s + sh]);
                    SA_HIP(hipMemcpy(d, p.data(), p.size() * sizeof(int), hipMemcpyHostToDevice));
                    perm.push_back(d);
                    int* pd = nullptr;
                    if (!pads.empty()) {
                        SA_HIP(hipMalloc((void**)&pd, pads.size() * sizeof(int)));
                        SA_HIP(hipMemcpy(pd, pads.data(), pads.size() * sizeof(int), hipMemcpyHostToDevice));
                    }
                    pad_rows.push_back(pd);
                    pad_count.push_back((int)pads.size());
                }
                h /= 2; wd /= 2;
            }
        }
        {
            std::vector<int> ident(B);
            for (size_t i = 0; i < B; ++i) ident[i] = (int)i;
            SA_HIP(hipMemcpy(slots_dev, ident.data(), B * sizeof(int), hipMemcpyHostToDevice));
            const void* tabs[17];
            for (int i = 0; i < 17; ++i) tabs[i] = w[SA_LW_EMB_TABLES + i];
            SA_HIP(hipMemcpy((void*)tabs_dev, tabs, sizeof(tabs), hipMemcpyHostToDevice));
            const int trc = launch_rope_table<T>(reinterpret_cast<const float*>(w[SA_LW_DEC_INVFREQ]), rope_cs, c.max_boxes, hd() / 2, 0);
            if (trc) return trc;
        }
        SA_HIP(hipHostMalloc((void**)&pinned, B * (MAX_PROMPT * 10 * sizeof(int) + (c.label_count + 6) * sizeof(float)) + 256, hipHostMallocDefault));
        int rrc = init_rings();
        if (rrc) return rrc;
        SA_HIP(hipDeviceSynchronize());
        return SA_OK;
    }
    ~LayoutModel() override {
        free_rings();
        for (int* pd : pad_rows) if (pd) (void)hipFree(pd);
        if (arena) (void)hipFree(arena);
        if (pinned) (void)hipHostFree(pinned);
    }

    template <int EPI>
    int gemm(const T* X, long ldx, const T* Wt, long ldw, T* C, long ldc, const T* bias, const T* R, long ldr, int M, int N, int K,
             hipStream_t s) {
        GemmArgs<T, T> a{X, ldx, Wt, ldw, C, ldc, bias, R, ldr, M, N, K};
        return launch_gemm<T, T, EPI>(a, s);
    }
    int layernorm(const T* in, int wi, int bi, T* out, const int* pm, long rows, int rpi, int C, float eps, hipStream_t s, int rpi_out = 0) {
        return lay::launch_layernorm<T>(in, W(wi), W(bi), out, pm, rows, rpi, C, eps, rpi_out, s);
    }

    int encode(const float* pixels, int B, hipStream_t s) override {
        if (B <= 0 || B > c.max_batch) return SA_ERR_ARG;
        int rc;
        int h = gh(), wd = gw(), dim = c.embed_dim;
        long rows = (long)B * h * wd;
        {
            if ((rc = lay::launch_patchify<T>(pixels, patch_rows, B, 3, c.img_h, c.img_w, c.patch, 64, s))) return rc;
            if ((rc = gemm<EPI_BIAS>(patch_rows, 64, W(SA_LW_PATCH_W), 64, hbuf, dim, W(SA_LW_PATCH_B), nullptr, 0, (int)rows, dim, 64, s))) return rc;
            if ((rc = layernorm(hbuf, SA_LW_EMB_LN_W, SA_LW_EMB_LN_B, x, nullptr, rows, h * wd, dim, 1e-5f, s))) return rc;
        }
        for (int st = 0; st < c.n_stages; ++st) {
            const int sb = stage_base[st], nh = c.heads[st], nkv = c.kv_heads[st], ws = c.window;
            if (dim / nh != 32) return SA_ERR_UNSUPPORTED;
            const int rpi = h * wd;
            if ((rc = lay::launch_add_rows<T>(x, W(sb + SA_LS_SINCOS), rows, rpi, dim, s))) return rc;
            const int qkv_n = (nh + 2 * nkv) * 32;
            for (int bi = 0; bi < c.depths[st]; ++bi) {
                const int wb = sb + SA_LS_COUNT + bi * SA_LB_COUNT;
                const bool shifted = (bi % 2 == 1) && std::min(h, wd) > ws;
                const int* pm = perm[2 * st + (shifted ? 1 : 0)];
                const int hp = grid_hp[st], wp = grid_wp[st], rpw = hp * wp;                  // the grid in whole windows
                const long rows_w = (long)B * rpw;
                const int pi = 2 * st + (shifted ? 1 : 0);
                if (pad_count[pi] && (rc = lay::launch_zero_rows<T>(hbuf, pad_rows[pi], pad_count[pi], B, rpw, dim, s))) return rc;
                if ((rc = layernorm(x, wb + SA_LB_LN1_W, wb + SA_LB_LN1_B, hbuf, pm, rows, rpi, dim, c.enc_eps, s, rpw))) return rc;
                if ((rc = gemm<EPI_BIAS>(hbuf, dim, W(wb + SA_LB_QKV_W), dim, qkv, qkv_n, W(wb + SA_LB_QKV_B), nullptr, 0, (int)rows_w, qkv_n, dim, s)))
                    return rc;
                const int nwx = wp / ws, nwy = hp / ws;
                if ((rc = lay::launch_window_attn<T>(qkv, reinterpret_cast<const float*>(w[wb + SA_LB_RELBIAS]), att, rows_w / 64, nh, nkv, nwx, nwy,
                                                     shifted ? ws / 2 : 0, ws, s))) return rc;
                if ((rc = gemm<EPI_BIAS>(att, dim, W(wb + SA_LB_PROJ_W), dim, hbuf, dim, W(wb + SA_LB_PROJ_B), nullptr, 0, (int)rows_w, dim, dim, s)))
                    return rc;
                if ((rc = lay::launch_gather_add<T>(x, hbuf, pm, rows, rpi, dim, rpw, s))) return rc;
                if ((rc = layernorm(x, wb + SA_LB_LN2_W, wb + SA_LB_LN2_B, hbuf, nullptr, rows, rpi, dim, c.enc_eps, s))) return rc;
                if ((rc = gemm<EPI_GELU>(hbuf, dim, W(wb + SA_LB_FC1_W), dim, mlp, 4 * dim, W(wb + SA_LB_FC1_B), nullptr, 0, (int)rows, 4 * dim, dim, s)))
                    return rc;
                if ((rc = gemm<EPI_RESIDUAL>(mlp, 4 * dim, W(wb + SA_LB_FC2_W), 4 * dim, x, dim, W(wb + SA_LB_FC2_B), x, dim, (int)rows, dim, 4 * dim,
                                             s))) return rc;
            }
            if (st + 1 < c.n_stages) {
                const long orows = rows / 4;
                if ((rc = lay::launch_merge_ln<T>(x, W(sb + SA_LS_MERGE_NORM_W), W(sb + SA_LS_MERGE_NORM_B), mlp, B, h, wd, dim, 1e-5f, s))) return rc;
                if ((rc = gemm<EPI_BIAS>(mlp, 4 * dim, W(sb + SA_LS_MERGE_RED_W), 4 * dim, x, 2 * dim, nullptr, nullptr, 0, (int)orows, 2 * dim,
                                         4 * dim, s))) return rc;
                rows = orows; h /= 2; wd /= 2; dim *= 2;
            }
        }
        if ((rc = lay::launch_add_rows<T>(x, W(SA_LW_POS_EMB), rows, h * wd, dim, s))) return rc;
        enc_rows_final = (int)rows;
        batch_encoded = batch_active = B;
        fed_ready = false;
        SA_HIP(hipMemcpyAsync(cross_map_dev, slots_dev, (size_t)B * sizeof(int), hipMemcpyDeviceToDevice, s));     // identity
        // cross-attention keys / values of every decoder layer (adetr/decoder.py:167-173: projected once, then cached)
        const int kv2 = 2 * kvd();
        for (int l = 0; l < c.dec_layers; ++l) {
            const int lb = dec_base + l * SA_LD_COUNT;
            T* dst = ckv + (size_t)l * c.max_batch * Lk * kv2;
            if ((rc = gemm<EPI_BIAS>(x, dim, W(lb + SA_LD_CKV_W), dim, dst, kv2, nullptr, nullptr, 0, (int)rows, kv2, dim, s))) return rc;
            if constexpr (sizeof(T) == 2)
                if ((rc = lay::launch_transpose_cross_v<T>(dst, cvT + (size_t)l * c.max_batch * kvd() * Lkp, B, Lk, c.dec_kv_heads, hd(), s))) return rc;
        }
        return (int)hipGetLastError();
    }

    int encoder_states(void* out, int B, hipStream_t s) override {
        if (B != batch_encoded) return SA_ERR_STATE;
        const size_t He = (size_t)c.embed_dim << (c.n_stages - 1);
        SA_HIP(hipMemcpyAsync(out, x, (size_t)enc_rows_final * He * sizeof(T), hipMemcpyDeviceToDevice, s));
        return SA_OK;
    }

    // Decoder rows != encoded images: row i cross-attends image src[i] (table recognition's cell pass). Synchronous, tiny.
    int select(const int32_t* src, int n) override {
        if (n <= 0 || n > c.max_batch || batch_encoded <= 0) return SA_ERR_ARG;
        for (int i = 0; i < n; ++i)
            if (src[i] < 0 || src[i] >= batch_encoded) return SA_ERR_ARG;
        SA_HIP(hipDeviceSynchronize());
        SA_HIP(hipMemcpy(cross_map_dev, src, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
        batch_active = n;
        fed_ready = false;
        return SA_OK;
    }

    // A decoder prompt of Tn tokens per row in ONE pass (positions 0 .. Tn - 1; the decode steps continue at Tn): GEMMs over B * Tn rows,
    // cross attention per (row, token), causal self-attention inside each row's prompt with the K / V rows written to the cache. What
    // the reference's first decoder call does with prefill = True (surya/table_rec/__init__.py:60-68). Activations live in the
    // encoder's idle MLP / qkv workspaces. Returns the heads' outputs of every row's LAST prompt token.
    int prefill(const int32_t* boxes, int B, int Tn, float* cls, float* box, hipStream_t s) override {
        if (B != batch_active) return SA_ERR_STATE;
        if (Tn < 1 || Tn > MAX_PROMPT || Tn > c.max_boxes) return SA_ERR_ARG;
        fed_ready = false;
        const int Hd = c.dec_hidden, I = c.dec_inter, nq = c.dec_heads, nkv = c.dec_kv_heads, d = hd(), kv = kvd();
        const int qkv_d = Hd + 2 * kv, rows = B * Tn, G = nq / nkv;
        if (G > 8 || (d != 64 && d != 32)) return SA_ERR_UNSUPPORTED;
        size_t off = 0;
        auto take = [&](size_t bytes) { size_t o = off; off = lalign(off + bytes); return o; };
        const size_t o_x = take((size_t)rows * Hd * sizeof(T)), o_h = take((size_t)rows * Hd * sizeof(T)), o_q = take((size_t)rows * Hd * sizeof(T));
        const size_t o_qkv = take((size_t)rows * qkv_d * sizeof(T)), o_at = take((size_t)rows * Hd * sizeof(T)), o_rs = take((size_t)rows * Hd * sizeof(T));
        const size_t o_ml = take((size_t)rows * I * sizeof(T));
        if (off > enc_mlp_bytes) return SA_ERR_ARG;                   // callers fall back to one decode step per prompt token
        char* wb = reinterpret_cast<char*>(mlp);
        T *px = (T*)(wb + o_x), *ph = (T*)(wb + o_h), *pq = (T*)(wb + o_q), *pqkv = (T*)(wb + o_qkv), *pat = (T*)(wb + o_at), *prs = (T*)(wb + o_rs),
          *pml = (T*)(wb + o_ml);
        off = 0;
        const size_t o_sc = take((size_t)rows * nq * cross_ranges * (d + 2) * sizeof(float)), o_mp = take((size_t)rows * sizeof(int)),
                     o_bx = take((size_t)rows * tokw() * sizeof(int));
        if (off > enc_qkv_bytes) return SA_ERR_ARG;
        char* qb = reinterpret_cast<char*>(qkv);
        float* pscr = (float*)(qb + o_sc);
        int *pmap = (int*)(qb + o_mp), *pbox = (int*)(qb + o_bx);
        int rc;
        int* hb = reinterpret_cast<int*>(pinned);
        memcpy(hb, boxes, (size_t)rows * tokw() * sizeof(int));
        SA_HIP(hipMemcpyAsync(pbox, hb, (size_t)rows * tokw() * sizeof(int), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(lay::expand_map_kernel, dim3(cdiv(rows, 256)), dim3(256), 0, s, cross_map_dev, pmap, B, Tn);
        if ((rc = lay::launch_embed<T>(c.family, pbox, tabs_dev, px, rows, Hd, c.box_embed, c.bbox_size, c.vocab, c.label_count, c.category_count,
                                       c.merge_count, s))) return rc;
        const float scale = 1.0f / sqrtf((float)d);
        const size_t layer_kv = (size_t)c.max_batch * nkv * c.max_boxes * d;
        auto norm = [&](const T* in, int wi, T* outp) { (void)lay::launch_rmsnorm<T>(in, W(wi), outp, rows, Hd, c.rms_eps, s); };
        for (int l = 0; l < c.dec_layers; ++l) {
            const int lb = dec_base + l * SA_LD_COUNT;
            norm(px, lb + SA_LD_CNORM, ph);
            if ((rc = gemm<EPI_BIAS>(ph, Hd, W(lb + SA_LD_CQ_W), Hd, pq, Hd, nullptr, nullptr, 0, rows, Hd, Hd, s))) return rc;
            if ((rc = lay::launch_cross_attn<T>(reinterpret_cast<const float*>(pq), 0, rows, ckv + (size_t)l * c.max_batch * Lk * 2 * kv,
                                                cvT + (size_t)l * c.max_batch * kv * Lkp, pscr, pat, pmap, rows, nq, nkv, d, Lk, scale, s))) return rc;
            if ((rc = gemm<EPI_RESIDUAL>(pat, Hd, W(lb + SA_LD_CO_W), Hd, prs, Hd, W(lb + SA_LD_CO_B), px, Hd, rows, Hd, Hd, s))) return rc;
            norm(prs, lb + SA_LD_TNORM, ph);
            if ((rc = gemm<EPI_BIAS>(ph, Hd, W(lb + SA_LD_QKV_W), Hd, pqkv, qkv_d, nullptr, nullptr, 0, rows, qkv_d, Hd, s))) return rc;
            if ((rc = lay::launch_prefill_attn<T>(pqkv, pat, kcache + (size_t)l * layer_kv, vcache + (size_t)l * layer_kv, rope_cs, B, Tn, nq, nkv, d,
                                                  c.max_boxes, scale, s))) return rc;
            // layout: + RAW layer input (double residual flow); table_rec: + the cross-attention output
            if ((rc = gemm<EPI_RESIDUAL>(pat, Hd, W(lb + SA_LD_TO_W), Hd, prs, Hd, W(lb + SA_LD_TO_B), c.family == SA_FAMILY_TABLE ? prs : px, Hd, rows, Hd,
                                         Hd, s))) return rc;
            norm(prs, lb + SA_LD_MNORM, ph);
            if ((rc = gemm<EPI_GEGLU>(ph, Hd, W(lb + SA_LD_GU_W), Hd, pml, I, nullptr, nullptr, 0, rows, 2 * I, Hd, s))) return rc;
            if ((rc = gemm<EPI_RESIDUAL>(pml, I, W(lb + SA_LD_DOWN_W), I, px, Hd, nullptr, prs, Hd, rows, Hd, I, s))) return rc;
        }
        if ((rc = lay::launch_heads<T>(px + (size_t)(Tn - 1) * Hd, (long)Tn * Hd, W(SA_LW_DEC_FNORM), W(SA_LW_DEC_LN_W), W(SA_LW_DEC_LN_B), W(SA_LW_DEC_LM_W),
                                       W(SA_LW_DEC_BB_W), W(SA_LW_DEC_BB_B), cls_dev, box_dev, B, Hd, c.label_count, c.rms_eps, c.ln_eps, s))) return rc;
        float* hc = reinterpret_cast<float*>(pinned + 256 + (size_t)c.max_batch * MAX_PROMPT * 10 * sizeof(int));
        float* hbx = hc + (size_t)c.max_batch * c.label_count;
        SA_HIP(hipMemcpyAsync(hc, cls_dev, (size_t)B * c.label_count * sizeof(float), hipMemcpyDeviceToHost, s));
        SA_HIP(hipMemcpyAsync(hbx, box_dev, (size_t)B * 6 * sizeof(float), hipMemcpyDeviceToHost, s));
        SA_HIP(hipStreamSynchronize(s));
        memcpy(cls, hc, (size_t)B * c.label_count * sizeof(float));
        memcpy(box, hbx, (size_t)B * 6 * sizeof(float));
        return SA_OK;
    }

    // Host-fed start of a decode step: the token rows go to the device, are embedded, and the first layer's cross_pre_norm is applied
    // (dx = embedding, dh = its norm). The fused heads kernel (lay::layout_heads_kernel<T, true>) leaves the same state for the
    // step after it, so only the FIRST step of a device-fed run comes through here.
    int start_step(const int32_t* boxes, int B, int pos, hipStream_t s) {
        const int Hd = c.dec_hidden;
        int* hb = reinterpret_cast<int*>(pinned);
        memcpy(hb, boxes, (size_t)B * tokw() * sizeof(int));
        SA_HIP(hipMemcpyAsync(boxes_dev, hb, (size_t)B * tokw() * sizeof(int), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(fill_int_kernel, dim3(cdiv(B, 64)), dim3(64), 0, s, len_dev, pos, B);
        int rc;
        if ((rc = lay::launch_embed<T>(c.family, boxes_dev, tabs_dev, dx, B, Hd, c.box_embed, c.bbox_size, c.vocab, c.label_count, c.category_count,
                                       c.merge_count, s))) return rc;
        return lay::launch_rmsnorm<T>(dx, W(dec_base + SA_LD_CNORM), dh, B, Hd, c.rms_eps, s);
    }

    // The decoder layers of one step for B rows: dx = the token embeddings, dh = cross_pre_norm(dx) of layer 0, len_dev = the cache
    // position of every row on entry; dx = the final layer's output on exit.
    int decode_layers(int B, hipStream_t s) {
        const int Hd = c.dec_hidden, I = c.dec_inter, nq = c.dec_heads, nkv = c.dec_kv_heads, d = hd(), kv = kvd();
        const int qkv_d = Hd + 2 * kv;
        int rc;
        const float scale = 1.0f / sqrtf((float)d);
        const size_t layer_kv = (size_t)c.max_batch * nkv * c.max_boxes * d;
        // Every M = B projection runs split-K (64 x 64 tiles over ~128-256 workgroups instead of 32) and hands its slabs to the
        // consumer: the cross-attention kernel sums the q slabs itself, the decode-attention kernel the qkv slabs, and
        // splitk_residual_adetr_norm_kernel folds reduce + bias + residual + the NEXT norm into one launch (r03: 1476 -> 680 us
        // per step of 32 pages, profiles/r03_g_layout_kernel_stats.md; the unsplit 64 x 32 launches ran 14 us each on 32 workgroups).
        auto splitk = [&](const T* A, int lda, const T* Wt, int N, int K, int& S) -> int {
            GemmArgs<T, T> a{A, lda, Wt, K, nullptr, 0, nullptr, nullptr, 0, B, N, K, 1, part};
            const int r = launch_gemm_splitk<T>(a, s);
            S = a.splitk;
            return r;
        };
        auto reduce_norm = [&](int S, const T* res, const T* bias, T* xo, const T* nw) {
            return lay::launch_reduce_norm<T>(part, S, B, res, bias, xo, nw, dh, Hd, c.rms_eps, s);
        };
        for (int l = 0; l < c.dec_layers; ++l) {
            const int lb = dec_base + l * SA_LD_COUNT;
            int S = 1;
            // cross attention (double residual flow, adetr/decoder.py:430-457): cross = o(attn(norm(x))) + x; dh = norm(x) on entry
            if ((rc = splitk(dh, Hd, W(lb + SA_LD_CQ_W), Hd, Hd, S))) return rc;
            if ((rc = lay::launch_cross_attn<T>(part, S, B, ckv + (size_t)l * c.max_batch * Lk * 2 * kv, cvT + (size_t)l * c.max_batch * kv * Lkp,
                                                cross_scratch, dattn, cross_map_dev, B, nq, nkv, d, Lk, scale, s))) return rc;
            if ((rc = splitk(dattn, Hd, W(lb + SA_LD_CO_W), Hd, Hd, S))) return rc;
            if ((rc = reduce_norm(S, dx, W(lb + SA_LD_CO_B), dres, W(lb + SA_LD_TNORM)))) return rc;            // dres = cross, dh = temporal_pre_norm(cross)
            // self attention on norm(cross); residual = o(attn) + RAW layer input
            {
                GemmArgs<T, T> a{dh, Hd, W(lb + SA_LD_QKV_W), Hd, nullptr, 0, nullptr, nullptr, 0, B, qkv_d, Hd, 1, part};
                if ((rc = launch_gemm_splitk<T>(a, s))) return rc;
                // the recogniser's decode-attention launcher (decode_attn.h); no host bound on the contexts here
                DecodeAttnArgs<T> da{part, a.splitk, W(SA_LW_DEC_ZERO_BIAS), dattn, kcache + (size_t)l * layer_kv, vcache + (size_t)l * layer_kv, slots_dev,
                                     len_dev, rope_cs, B, nq, nkv, d, c.max_boxes, scale};
                if ((rc = launch_decode_attn<T>(da, s))) return rc;
            }
            if ((rc = splitk(dattn, Hd, W(lb + SA_LD_TO_W), Hd, Hd, S))) return rc;
            // layout: + RAW layer input (double residual flow); table_rec: + the cross-attention output (adetr/decoder.py:395-417)
            if ((rc = reduce_norm(S, c.family == SA_FAMILY_TABLE ? dres : dx, W(lb + SA_LD_TO_B), dres, W(lb + SA_LD_MNORM)))) return rc; // dh = channel_pre_norm(residual)
            // MLP: x = down(gelu_tanh(gate(n)) * up(n)) + residual; dh <- the next layer's cross_pre_norm(x)
            if ((rc = gemm<EPI_GEGLU>(dh, Hd, W(lb + SA_LD_GU_W), Hd, dmlp, I, nullptr, nullptr, 0, B, 2 * I, Hd, s))) return rc;
            if ((rc = splitk(dmlp, I, W(lb + SA_LD_DOWN_W), Hd, I, S))) return rc;
            if ((rc = reduce_norm(S, dres, nullptr, dx, l + 1 < c.dec_layers ? W(lb + SA_LD_COUNT + SA_LD_CNORM) : nullptr))) return rc;
        }
        return (int)hipGetLastError();
    }

    int decode_step(const int32_t* boxes, int B, int pos, float* cls, float* box, hipStream_t s) override {
        if (B != batch_active) return SA_ERR_STATE;
        if (pos < 0 || pos >= c.max_boxes) return SA_ERR_ARG;
        const int Hd = c.dec_hidden;
        int rc;
        fed_ready = false;
        if ((rc = start_step(boxes, B, pos, s))) return rc;
        if ((rc = decode_layers(B, s))) return rc;
        if ((rc = lay::launch_heads<T>(dx, (long)Hd, W(SA_LW_DEC_FNORM), W(SA_LW_DEC_LN_W), W(SA_LW_DEC_LN_B), W(SA_LW_DEC_LM_W), W(SA_LW_DEC_BB_W),
                                       W(SA_LW_DEC_BB_B), cls_dev, box_dev, B, Hd, c.label_count, c.rms_eps, c.ln_eps, s))) return rc;
        float* hc = reinterpret_cast<float*>(pinned + 256 + (size_t)c.max_batch * MAX_PROMPT * 10 * sizeof(int));
        float* hbx = hc + (size_t)c.max_batch * c.label_count;
        SA_HIP(hipMemcpyAsync(hc, cls_dev, (size_t)B * c.label_count * sizeof(float), hipMemcpyDeviceToHost, s));
        SA_HIP(hipMemcpyAsync(hbx, box_dev, (size_t)B * 6 * sizeof(float), hipMemcpyDeviceToHost, s));
        SA_HIP(hipStreamSynchronize(s));
        memcpy(cls, hc, (size_t)B * c.label_count * sizeof(float));
        memcpy(box, hbx, (size_t)B * 6 * sizeof(float));
        return SA_OK;
    }

    // ------------------------------------------------------------------------------------------------ device-fed decode steps (round 4)
    // n_steps decode steps whose fed-back tokens never leave the device (lay::layout_heads_kernel<T, true>), recorded in ring `ring`
    // ([step][row] class logits / boxes / fed tokens); one D2H copy + event at the end, no host synchronisation: the caller enqueues
    // the next run before it waits for this one. With surya_set_tuning("graph", 1) a run is replayed as a hipGraph once its (rows,
    // steps) shape has been seen twice (the cache position lives in len_dev, so it is not part of the shape); measured slower, off by default.
    static constexpr int RING_STEPS = 16;
    float *cls_ring = nullptr, *box_ring = nullptr;
    int *tok_ring = nullptr, *page_sizes_dev = nullptr;
    char* ring_host = nullptr;                   // pinned: [2] x (cls | box | tok) of RING_STEPS steps
    size_t ring_cls = 0, ring_box = 0, ring_tok = 0;     // elements per ring
    hipEvent_t ev_ring[2] = {nullptr, nullptr}, gev_in = nullptr, gev_out = nullptr;
    hipStream_t gstream = nullptr;
    std::map<long, hipGraphExec_t> graphs;
    std::set<long> seen_keys;
    bool use_graph = true, fed_ready = false;
    int fed_rows = 0, fed_pos = 0;
    surya_layout_feedback fbcfg{};
    bool have_sizes = false, fb_set = false;
    int graph_epoch = 0;
    void drop_graphs() {
        for (auto& kv : graphs) (void)hipGraphExecDestroy(kv.second);
        graphs.clear(); seen_keys.clear();
    }

    int init_rings() {
        const size_t B = c.max_batch;
        ring_cls = (size_t)RING_STEPS * B * c.label_count; ring_box = (size_t)RING_STEPS * B * 6; ring_tok = (size_t)RING_STEPS * B * 10;
        SA_HIP(hipMalloc((void**)&cls_ring, 2 * ring_cls * sizeof(float)));
        SA_HIP(hipMalloc((void**)&box_ring, 2 * ring_box * sizeof(float)));
        SA_HIP(hipMalloc((void**)&tok_ring, 2 * ring_tok * sizeof(int)));
        SA_HIP(hipMalloc((void**)&page_sizes_dev, B * 2 * sizeof(int)));
        SA_HIP(hipHostMalloc((void**)&ring_host, 2 * (ring_cls + ring_box + ring_tok) * 4 + B * 2 * sizeof(int), hipHostMallocDefault));
        for (auto& e : ev_ring) SA_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        SA_HIP(hipEventCreateWithFlags(&gev_in, hipEventDisableTiming));
        SA_HIP(hipEventCreateWithFlags(&gev_out, hipEventDisableTiming));
        SA_HIP(hipStreamCreateWithFlags(&gstream, hipStreamNonBlocking));
        return SA_OK;
    }
    void free_rings() {
        for (auto& kv : graphs) (void)hipGraphExecDestroy(kv.second);
        graphs.clear();
        if (cls_ring) (void)hipFree(cls_ring);
        if (box_ring) (void)hipFree(box_ring);
        if (tok_ring) (void)hipFree(tok_ring);
        if (page_sizes_dev) (void)hipFree(page_sizes_dev);
        if (ring_host) (void)hipHostFree(ring_host);
        for (auto& e : ev_ring) if (e) (void)hipEventDestroy(e);
        if (gev_in) (void)hipEventDestroy(gev_in);
        if (gev_out) (void)hipEventDestroy(gev_out);
        if (gstream) (void)hipStreamDestroy(gstream);
    }

    int set_feedback(const surya_layout_feedback* fb, int B, hipStream_t s) override {
        if (!fb) return SA_ERR_ARG;
        if (B <= 0 || B > c.max_batch) return SA_ERR_ARG;
        if (c.label_count + 6 > 64) return SA_ERR_UNSUPPORTED;
        if (c.family == SA_FAMILY_TABLE && fb->head_widths[0] + fb->head_widths[1] + fb->head_widths[2] + fb->head_widths[3] != c.label_count) return SA_ERR_SHAPE;
        if (c.family == SA_FAMILY_TABLE && (fb->head_widths[2] != 1 || fb->head_widths[0] < 1 || fb->head_widths[1] < 1 || fb->head_widths[3] < 1)) return SA_ERR_SHAPE;
        const bool changed = memcmp(&fbcfg, fb, sizeof(int32_t) * 7) != 0 || have_sizes != (fb->page_sizes != nullptr);
        fbcfg = *fb;
        have_sizes = fb->page_sizes != nullptr;
        fbcfg.page_sizes = nullptr;
        if (changed) drop_graphs();                              // captured runs hold the old rule's constants
        fb_set = true;
        if (have_sizes) {
            int* hs = reinterpret_cast<int*>(ring_host + 2 * (ring_cls + ring_box + ring_tok) * 4);
            SA_HIP(hipStreamSynchronize(s));                     // an earlier upload from this staging area may still be in flight
            memcpy(hs, fb->page_sizes, (size_t)B * 2 * sizeof(int));
            SA_HIP(hipMemcpyAsync(page_sizes_dev, hs, (size_t)B * 2 * sizeof(int), hipMemcpyHostToDevice, s));
        }
        return SA_OK;
    }

    int fed_steps_eager(int B, int n_steps, int ring, hipStream_t s) {
        const int Hd = c.dec_hidden;
        int rc;
        lay::LayoutFeedback fb;
        fb.boxes = boxes_dev; fb.len = len_dev; fb.page_sizes = have_sizes ? page_sizes_dev : nullptr;
        fb.family = c.family; fb.tokw = tokw(); fb.bbox_size = c.bbox_size; fb.vocab = c.vocab; fb.skew_scaler = fbcfg.skew_scaler;
        fb.relabel_a = fbcfg.relabel_ids[0]; fb.relabel_b = fbcfg.relabel_ids[1];
        fb.wcat = fbcfg.head_widths[0]; fb.wmer = fbcfg.head_widths[1]; fb.whdr = fbcfg.head_widths[3];
        fb.box_embed = c.box_embed; fb.category_count = c.category_count; fb.merge_count = c.merge_count; fb.embed_labels = c.label_count;
        for (int k = 0; k < n_steps; ++k) {
            if ((rc = decode_layers(B, s))) return rc;
            const size_t slot = (size_t)ring * RING_STEPS + k;
            fb.tok_ring = tok_ring + slot * c.max_batch * 10;
            hipLaunchKernelGGL((lay::layout_heads_kernel<T, true>), dim3(B), dim3(256), (size_t)Hd * 4, s, dx, W(SA_LW_DEC_FNORM), W(SA_LW_DEC_LN_W),
                               W(SA_LW_DEC_LN_B), W(SA_LW_DEC_LM_W), W(SA_LW_DEC_BB_W), W(SA_LW_DEC_BB_B),
                               cls_ring + slot * c.max_batch * c.label_count, box_ring + slot * c.max_batch * 6, Hd, c.label_count, c.rms_eps,
                               c.ln_eps, (long)Hd, fb, tabs_dev, dx, W(dec_base + SA_LD_CNORM), dh);
            if ((rc = (int)hipGetLastError())) return rc;
        }
        return SA_OK;
    }

    int decode_steps(const int32_t* boxes, int B, int pos0, int n_steps, int ring, hipStream_t s) override {
        if (B != batch_active) return SA_ERR_STATE;
        if (n_steps < 1 || n_steps > RING_STEPS || ring < 0 || ring > 1 || pos0 < 0 || pos0 + n_steps > c.max_boxes) return SA_ERR_ARG;
        if (!fb_set) return SA_ERR_STATE;                       // surya_layout_set_feedback first
        if (graph_epoch != tuning_epoch()) { drop_graphs(); graph_epoch = tuning_epoch(); }      // split-K shapes follow the tuning knobs
        int rc;
        if (boxes) {
            if ((rc = start_step(boxes, B, pos0, s))) return rc;
        } else if (!fed_ready || fed_rows != B || fed_pos != pos0) {
            return SA_ERR_STATE;                                 // nothing on the device to continue from at this position
        }
        fed_ready = false;
        const long key = (long)B * 64 + n_steps + (long)ring * (1L << 40);
        bool replayed = false;
        // hipGraph replay is opt-in (surya_set_tuning("graph", 1)), as for the recogniser: a run is ~1400 kernel nodes and the replay measured
        // SLOWER than plain launches enqueued ahead of the device (gpurun r04e / r04f, 32 pages: 628 vs 552 us per step; host-fed loop 570-587)
        if (use_graph && tuning().graph == 1 && !gemm_profiler().enabled) {
            auto it = graphs.find(key);
            if (it == graphs.end() && seen_keys.count(key)) {
                hipGraph_t g = nullptr;
                SA_HIP(hipStreamBeginCapture(gstream, hipStreamCaptureModeThreadLocal));
                rc = fed_steps_eager(B, n_steps, ring, gstream);
                hipError_t e = hipStreamEndCapture(gstream, &g);
                hipGraphExec_t ex = nullptr;
                if (!rc && e == hipSuccess && g) e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
                if (g) (void)hipGraphDestroy(g);
                if (rc || e != hipSuccess || !ex) { (void)hipGetLastError(); use_graph = false; }
                else it = graphs.emplace(key, ex).first;
            }
            seen_keys.insert(key);                               // the first run of a shape is eager: one-time attribute calls happen there
            if (it != graphs.end()) {
                SA_HIP(hipEventRecord(gev_in, s));
                SA_HIP(hipStreamWaitEvent(gstream, gev_in, 0));
                SA_HIP(hipGraphLaunch(it->second, gstream));
                SA_HIP(hipEventRecord(gev_out, gstream));
                SA_HIP(hipStreamWaitEvent(s, gev_out, 0));
                replayed = true;
            }
        }
        if (!replayed && (rc = fed_steps_eager(B, n_steps, ring, s))) return rc;
        const size_t mb = c.max_batch, off = (size_t)ring * RING_STEPS;
        float* hc = reinterpret_cast<float*>(ring_host) + (size_t)ring * (ring_cls + ring_box + ring_tok);
        float* hb = hc + ring_cls;
        int* ht = reinterpret_cast<int*>(hb + ring_box);
        SA_HIP(hipMemcpyAsync(hc, cls_ring + off * mb * c.label_count, (size_t)n_steps * mb * c.label_count * sizeof(float), hipMemcpyDeviceToHost, s));
        SA_HIP(hipMemcpyAsync(hb, box_ring + off * mb * 6, (size_t)n_steps * mb * 6 * sizeof(float), hipMemcpyDeviceToHost, s));
        SA_HIP(hipMemcpyAsync(ht, tok_ring + off * mb * 10, (size_t)n_steps * mb * 10 * sizeof(int), hipMemcpyDeviceToHost, s));
        SA_HIP(hipEventRecord(ev_ring[ring], s));
        fed_ready = true; fed_rows = B; fed_pos = pos0 + n_steps;
        return SA_OK;
    }

    int wait_steps(int ring, int B, int n_steps, float* cls, float* box, int32_t* tok) override {
        if (ring < 0 || ring > 1 || n_steps < 1 || n_steps > RING_STEPS || B < 1 || B > c.max_batch) return SA_ERR_ARG;
        SA_HIP(hipEventSynchronize(ev_ring[ring]));
        const size_t mb = c.max_batch;
        const float* hc = reinterpret_cast<const float*>(ring_host) + (size_t)ring * (ring_cls + ring_box + ring_tok);
        const float* hb = hc + ring_cls;
        const int* ht = reinterpret_cast<const int*>(hb + ring_box);
        const int tw = tokw();
        for (int k = 0; k < n_steps; ++k) {                      // device rings are [step][max_batch]; the caller's arrays [step][B]
            memcpy(cls + (size_t)k * B * c.label_count, hc + (size_t)k * mb * c.label_count, (size_t)B * c.label_count * sizeof(float));
            memcpy(box + (size_t)k * B * 6, hb + (size_t)k * mb * 6, (size_t)B * 6 * sizeof(float));
            memcpy(tok + (size_t)k * B * tw, ht + (size_t)k * mb * 10, (size_t)B * tw * sizeof(int));          // rows packed at the token width
        }
        return SA_OK;
    }
};

}  // namespace sa

namespace sa {
// EPI_GEGLU for surya_op_gemm (rec_model.hip): the ADETR MLP's gate|up GEMM exactly as LayoutModel::gemm<EPI_GEGLU> launches it
int op_gemm_geglu(int dtype, const void* X, long ldx, const void* W, long ldw, void* C, long ldc, int M, int N, int K, hipStream_t s) {
    if (dtype == SA_DTYPE_F32) {
        GemmArgs<float, float> a{(const float*)X, ldx, (const float*)W, ldw, (float*)C, ldc, nullptr, nullptr, 0, M, N, K};
        return launch_gemm<float, float, EPI_GEGLU>(a, s);
    }
    if (dtype == SA_DTYPE_BF16) {
        GemmArgs<bf16_t, bf16_t> a{(const bf16_t*)X, ldx, (const bf16_t*)W, ldw, (bf16_t*)C, ldc, nullptr, nullptr, 0, M, N, K};
        return launch_gemm<bf16_t, bf16_t, EPI_GEGLU>(a, s);
    }
    if (dtype == SA_DTYPE_F16) {
        GemmArgs<fp16_t, fp16_t> a{(const fp16_t*)X, ldx, (const fp16_t*)W, ldw, (fp16_t*)C, ldc, nullptr, nullptr, 0, M, N, K};
        return launch_gemm<fp16_t, fp16_t, EPI_GEGLU>(a, s);
    }
    return SA_ERR_UNSUPPORTED;
}

// launch_decode_attn (decode_attn.h) in fp16: the fourth-version kernel on v_mfma_f32_32x32x16_f16 at the head shapes of this family's decoders,
// in this code object beside LayoutModel<fp16_t> (d = 128, the recogniser's, is built in rec_model_f16.hip). Tuning::dattn_db as in bf16; no third version.
template <int D>
static int decode_attn_flash_f16(const DecodeAttnArgs<fp16_t>& a, hipStream_t s) {
    const Tuning& t = tuning();
    if (t.dattn_db == 1 || (t.dattn_db == 0 && !t.graph && a.ctx_bound > 128 && a.rows * a.nkv <= 256))
        return decode_attn_as<decode_attn_flash2_kernel<D, 8, true, fp16_t>>(a, decode_attn_flash2_lds<D, 8, true>(), s, a.out8, a.sout, a.srows);
    return decode_attn_as<decode_attn_flash2_kernel<D, 8, false, fp16_t>>(a, decode_attn_flash2_lds<D, 8, false>(), s, a.out8, a.sout, a.srows);
}
template <>
int launch_decode_attn<fp16_t>(const DecodeAttnArgs<fp16_t>& a, hipStream_t s) {
    const int G = a.nq / a.nkv;
    if (a.out8 || G < 1 || G > 8 || a.nq % a.nkv) return SA_ERR_UNSUPPORTED;
    if (a.d == 64) return decode_attn_flash_f16<64>(a, s);
    if (a.d == 32) return decode_attn_flash_f16<32>(a, s);
    if (a.d == 128) return decode_attn_f16_d128(a, s);       // the recogniser's head shape: built beside RecModel<fp16_t> (rec_model_f16.hip)
    return SA_ERR_UNSUPPORTED;
}
}  // namespace sa

using namespace sa;
struct surya_layout { std::unique_ptr<LayoutBase> impl; };

extern "C" {

int surya_layout_create(const surya_layout_config* cfg, const void* const* weights, int n_weights, surya_layout** out) {
    if (!cfg || !weights || !out) return SA_ERR_ARG;
    if (cfg->n_stages < 1 || cfg->n_stages > 8 || cfg->patch * cfg->patch * 3 > 64 || cfg->embed_dim % 64 || cfg->window != 8) return SA_ERR_UNSUPPORTED;
    if (cfg->img_h % cfg->patch || cfg->img_w % cfg->patch || cfg->dec_hidden % 64 || cfg->dec_inter % 64 || cfg->dec_heads % cfg->dec_kv_heads)
        return SA_ERR_SHAPE;
    if (cfg->max_batch <= 0 || cfg->max_boxes <= 0 || cfg->label_count <= 0) return SA_ERR_ARG;
    if (cfg->vocab <= cfg->bbox_size) return SA_ERR_SHAPE;       // box_embed / table_embed clamp corners to [0, bbox_size] and index [vocab]-row tables
    if (cfg->family != SA_FAMILY_LAYOUT && cfg->family != SA_FAMILY_TABLE) return SA_ERR_ARG;
    if (cfg->family == SA_FAMILY_TABLE &&
        (cfg->box_embed <= 0 || cfg->box_embed >= cfg->dec_hidden || cfg->category_count <= 0 || cfg->merge_count <= 0)) return SA_ERR_ARG;
    for (int i = 0; i < n_weights; ++i)
        if (!weights[i]) return SA_ERR_ARG;
    auto* h = new surya_layout();
    int rc;
    if (cfg->dtype == SA_DTYPE_F32) {
        auto m = std::make_unique<LayoutModel<float>>();
        rc = m->init(*cfg, weights, n_weights);
        h->impl = std::move(m);
    } else if (cfg->dtype == SA_DTYPE_BF16) {
        auto m = std::make_unique<LayoutModel<bf16_t>>();
        rc = m->init(*cfg, weights, n_weights);
        h->impl = std::move(m);
    } else if (cfg->dtype == SA_DTYPE_F16) {
        auto m = std::make_unique<LayoutModel<fp16_t>>();
        rc = m->init(*cfg, weights, n_weights);
        h->impl = std::move(m);
    } else {
        rc = SA_ERR_UNSUPPORTED;
    }
    if (rc) { delete h; return rc; }
    *out = h;
    return SA_OK;
}

int surya_layout_destroy(surya_layout* h) {
    if (!h) return SA_ERR_ARG;
    (void)hipDeviceSynchronize();
    delete h;
    return SA_OK;
}

int surya_layout_encode(surya_layout* h, const float* pixel_values, int batch, void* stream) {
    if (!h || !pixel_values) return SA_ERR_ARG;
    return h->impl->encode(pixel_values, batch, (hipStream_t)stream);
}

int surya_layout_decode_step(surya_layout* h, const int32_t* boxes, int batch, int position, float* class_logits, float* bbox, void* stream) {
    if (!h || !boxes || !class_logits || !bbox) return SA_ERR_ARG;
    return h->impl->decode_step(boxes, batch, position, class_logits, bbox, (hipStream_t)stream);
}

int surya_layout_prefill(surya_layout* h, const int32_t* boxes, int batch, int n_tokens, float* class_logits, float* bbox, void* stream) {
    if (!h || !boxes || !class_logits || !bbox) return SA_ERR_ARG;
    return h->impl->prefill(boxes, batch, n_tokens, class_logits, bbox, (hipStream_t)stream);
}

int surya_layout_set_feedback(surya_layout* h, const surya_layout_feedback* fb, int batch, void* stream) {
    if (!h || !fb) return SA_ERR_ARG;
    return h->impl->set_feedback(fb, batch, (hipStream_t)stream);
}

int surya_layout_decode_steps(surya_layout* h, const int32_t* boxes, int batch, int position, int n_steps, int ring, void* stream) {
    if (!h) return SA_ERR_ARG;
    return h->impl->decode_steps(boxes, batch, position, n_steps, ring, (hipStream_t)stream);
}

int surya_layout_wait_steps(surya_layout* h, int ring, int batch, int n_steps, float* class_logits, float* bbox, int32_t* fed_tokens) {
    if (!h || !class_logits || !bbox || !fed_tokens) return SA_ERR_ARG;
    return h->impl->wait_steps(ring, batch, n_steps, class_logits, bbox, fed_tokens);
}

int surya_layout_select(surya_layout* h, const int32_t* src_index, int n) {
    if (!h || !src_index) return SA_ERR_ARG;
    return h->impl->select(src_index, n);
}

int surya_layout_encoder_states(surya_layout* h, void* out, int batch, void* stream) {
    if (!h || !out) return SA_ERR_ARG;
    return h->impl->encoder_states(out, batch, (hipStream_t)stream);
}

int surya_layout_preprocess(const uint8_t* pages, size_t pages_bytes, const void* descs, int n, int pixel_stride, const float* mean,
                            const float* std, int out_h, int out_w, float* pixel_values, void* stream) {
    return sa::lprep::run(pages, pages_bytes, reinterpret_cast<const sa::lprep::PageDesc*>(descs), n, pixel_stride, mean, std, out_h,
                          out_w, pixel_values, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------ op level
// Every kernel of the family alone, through the launch functions LayoutModel calls (sa::lay::launch_*). Caller-owned device memory, enqueue only.
// The bodies (lay_op_*) take all three dtypes; the exported entries over them are at the end of the file.
#define SA_LAY_DT(CALL_F32, CALL_16)                   \
    if (dtype == SA_DTYPE_F32) { typedef float T; return CALL_F32; }     \
    if (dtype == SA_DTYPE_BF16) { typedef bf16_t T; return CALL_16; }   \
    if (dtype == SA_DTYPE_F16) { typedef fp16_t T; return CALL_16; }    \
    return SA_ERR_UNSUPPORTED;
#define SA_LAY_BOTH(CALL) SA_LAY_DT(CALL, CALL)

int surya_lay_window_tables(int h, int w, int window, int shift, int32_t* perm, int32_t* pad_rows, int32_t* n_pad, int32_t* padded_hw,
                            int32_t* shift_used) {
    std::vector<int> p, pads;
    int hp = 0, wp = 0, sh = 0;
    const int rc = lay::window_tables(h, w, window, shift, p, pads, hp, wp, sh);
    if (rc) return rc;
    if (perm) memcpy(perm, p.data(), p.size() * sizeof(int));
    if (pad_rows && !pads.empty()) memcpy(pad_rows, pads.data(), pads.size() * sizeof(int));
    if (n_pad) *n_pad = (int)pads.size();
    if (padded_hw) { padded_hw[0] = hp; padded_hw[1] = wp; }
    if (shift_used) *shift_used = sh;
    return SA_OK;
}

int surya_lay_cross_plan(int Lk, int32_t* chunk, int32_t* ranges, int32_t* Lkp) {
    if (Lk < 1) return SA_ERR_ARG;
    const lay::CrossPlan cp = lay::cross_plan(Lk);
    if (chunk) *chunk = cp.chunk;
    if (ranges) *ranges = cp.ranges;
    if (Lkp) *Lkp = cp.Lkp;
    return SA_OK;
}

static int lay_op_layernorm(int dtype, const void* x, const void* w, const void* b, void* y, const int32_t* perm, long rows, int rows_per_image,
                           int C, float eps, int rows_per_image_out, void* stream) {
    if (!x || !w || !b || !y || rows <= 0 || rows_per_image <= 0 || C <= 0 || C % 4) return SA_ERR_ARG;
    SA_LAY_BOTH(lay::launch_layernorm<T>((const T*)x, (const T*)w, (const T*)b, (T*)y, perm, rows, rows_per_image, C, eps, rows_per_image_out,
                                         (hipStream_t)stream))
}

static int lay_op_window_attn(int dtype, const void* qkv, const float* bias, void* out, long windows, int nh, int nkv, int nwx, int nwy, int shift,
                             int ws, void* stream) {
    if (!qkv || !bias || !out || windows <= 0 || nh <= 0 || nkv <= 0 || nwx <= 0 || nwy <= 0 || shift < 0) return SA_ERR_ARG;
    if (ws != 8 || shift >= ws) return SA_ERR_UNSUPPORTED;           // 64 tokens per window, head dim 32
    SA_LAY_BOTH(lay::launch_window_attn<T>((const T*)qkv, bias, (T*)out, windows, nh, nkv, nwx, nwy, shift, ws, (hipStream_t)stream))
}

static int lay_op_merge_ln(int dtype, const void* x, const void* w, const void* b, void* y, int B, int H, int W, int C, float eps, void* stream) {
    if (!x || !w || !b || !y || B <= 0 || H < 2 || W < 2 || C <= 0) return SA_ERR_ARG;
    if (H % 2 || W % 2 || C % 4) return SA_ERR_SHAPE;
    SA_LAY_BOTH(lay::launch_merge_ln<T>((const T*)x, (const T*)w, (const T*)b, (T*)y, B, H, W, C, eps, (hipStream_t)stream))
}

static int lay_op_rows(int dtype, int kind, void* dst, const void* src, const int32_t* index, const int32_t* dims, void* stream) {
    if (!dst || !dims) return SA_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    switch (kind) {
        case SA_LAY_PATCHIFY: {
            const int B = dims[0], Cc = dims[1], H = dims[2], Wd = dims[3], P = dims[4], Kpad = dims[5];
            if (!src || B <= 0 || Cc <= 0 || P <= 0 || H <= 0 || Wd <= 0 || Kpad < Cc * P * P) return SA_ERR_ARG;
            if (H % P || Wd % P) return SA_ERR_SHAPE;
            SA_LAY_BOTH(lay::launch_patchify<T>((const float*)src, (T*)dst, B, Cc, H, Wd, P, Kpad, s))
        }
        case SA_LAY_ADD_ROWS: {
            if (!src || dims[0] <= 0 || dims[1] <= 0 || dims[2] <= 0 || dims[2] % 4) return SA_ERR_ARG;
            SA_LAY_BOTH(lay::launch_add_rows<T>((T*)dst, (const T*)src, dims[0], dims[1], dims[2], s))
        }
        case SA_LAY_ZERO_ROWS: {
            if (!index || dims[0] <= 0 || dims[1] <= 0 || dims[2] <= 0 || dims[3] <= 0 || dims[3] % 4) return SA_ERR_ARG;
            SA_LAY_BOTH(lay::launch_zero_rows<T>((T*)dst, index, dims[1], dims[0], dims[2], dims[3], s))
        }
        case SA_LAY_GATHER_ADD: {
            if (!src || !index || dims[0] <= 0 || dims[1] <= 0 || dims[2] <= 0 || dims[2] % 4 || dims[3] < 0) return SA_ERR_ARG;
            SA_LAY_BOTH(lay::launch_gather_add<T>((T*)dst, (const T*)src, index, dims[0], dims[1], dims[2], dims[3], s))
        }
    }
    return SA_ERR_ARG;
}

static int lay_op_cross_attn(int dtype, int head_dim, const void* qpart, int S, int M, const void* kv, int n_images, const int32_t* item_map,
                            void* out, float* scratch, void* vT, int nq, int nkv, int Lk, float scale, void* stream) {
    if (!qpart || !kv || !item_map || !out || M <= 0 || n_images <= 0 || nq <= 0 || nkv <= 0 || Lk <= 0) return SA_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == SA_DTYPE_F32) {
        if (!scratch) return SA_ERR_ARG;
        return lay::launch_cross_attn<float>((const float*)qpart, S, M, (const float*)kv, nullptr, scratch, (float*)out, item_map, M, nq, nkv, head_dim, Lk,
                                             scale, s);
    }
    if (dtype != SA_DTYPE_BF16 && dtype != SA_DTYPE_F16) return SA_ERR_UNSUPPORTED;
    if (!vT) return SA_ERR_ARG;
    if (head_dim != 64 && head_dim != 32) return SA_ERR_UNSUPPORTED;
#define SA_LAY_CROSS16(T)                                                                                                                  \
    {                                                                                                                                      \
        const int rc = lay::launch_transpose_cross_v<T>((const T*)kv, (T*)vT, n_images, Lk, nkv, head_dim, s);                             \
        if (rc) return rc;                                                                                                                 \
        return lay::launch_cross_attn<T>((const float*)qpart, S, M, (const T*)kv, (const T*)vT, nullptr, (T*)out, item_map, M, nq, nkv, head_dim, \
                                         Lk, scale, s);                                                                                    \
    }
    if (dtype == SA_DTYPE_BF16) SA_LAY_CROSS16(bf16_t)
    SA_LAY_CROSS16(fp16_t)
#undef SA_LAY_CROSS16
}

static int lay_op_rmsnorm(int dtype, const void* x, const void* w, void* y, int rows, int C, float eps, void* stream) {
    if (!x || !w || !y || rows <= 0 || C <= 0 || C % 4) return SA_ERR_ARG;
    SA_LAY_BOTH(lay::launch_rmsnorm<T>((const T*)x, (const T*)w, (T*)y, rows, C, eps, (hipStream_t)stream))
}

static int lay_op_reduce_norm(int dtype, const float* part, int S, int M, const void* res, const void* bias, void* x_out, const void* w, void* y,
                             int H, float eps, void* stream) {
    if (!part || !res || !x_out || M <= 0 || (w && !y)) return SA_ERR_ARG;
    SA_LAY_BOTH(lay::launch_reduce_norm<T>(part, S, M, (const T*)res, (const T*)bias, (T*)x_out, (const T*)w, (T*)y, H, eps, (hipStream_t)stream))
}

static int lay_op_prefill_attn(int dtype, int head_dim, const void* qkv, void* out, void* kcache, void* vcache, const float* rope_cs, int B, int Tn,
                              int nq, int nkv, int Tmax, float scale, void* stream) {
    if (!qkv || !out || !kcache || !vcache || !rope_cs || B <= 0 || nq <= 0 || nkv <= 0) return SA_ERR_ARG;
    SA_LAY_BOTH(lay::launch_prefill_attn<T>((const T*)qkv, (T*)out, (T*)kcache, (T*)vcache, (const float2*)rope_cs, B, Tn, nq, nkv, head_dim, Tmax, scale,
                                            (hipStream_t)stream))
}

static int lay_op_embed(int dtype, int family, const int32_t* tokens, const void* const* tabs, void* x, int rows, int Hd, int box_embed,
                       int bbox_size, int vocab, int label_count, int category_count, int merge_count, void* stream) {
    if (!tokens || !tabs || !x || rows <= 0 || Hd <= 0 || bbox_size <= 0) return SA_ERR_ARG;
    if (vocab <= bbox_size) return SA_ERR_SHAPE;                   // corners clamp to [0, bbox_size] and index [vocab]-row tables (surya_layout_create)
    if (family == SA_FAMILY_TABLE) {
        if (box_embed <= 0 || box_embed >= Hd || category_count <= 0 || merge_count <= 0) return SA_ERR_ARG;
    } else if (family != SA_FAMILY_LAYOUT || label_count <= 0) return SA_ERR_ARG;
    SA_LAY_BOTH(lay::launch_embed<T>(family, tokens, (const T* const*)tabs, (T*)x, rows, Hd, box_embed, bbox_size, vocab, label_count, category_count,
                                     merge_count, (hipStream_t)stream))
}

static int lay_op_heads(int dtype, const void* x, long ldx, const void* fnorm_w, const void* ln_w, const void* ln_b, const void* lm_w, const void* bb_w,
                       const void* bb_b, float* class_logits, float* bbox, int B, int Hd, int label_count, float rms_eps, float ln_eps, void* stream) {
    if (!x || !fnorm_w || !ln_w || !ln_b || !lm_w || !bb_w || !bb_b || !class_logits || !bbox || B <= 0 || Hd <= 0 || label_count <= 0 || ldx < Hd)
        return SA_ERR_ARG;
    SA_LAY_BOTH(lay::launch_heads<T>((const T*)x, ldx, (const T*)fnorm_w, (const T*)ln_w, (const T*)ln_b, (const T*)lm_w, (const T*)bb_w, (const T*)bb_b,
                                     class_logits, bbox, B, Hd, label_count, rms_eps, ln_eps, (hipStream_t)stream))
}
#undef SA_LAY_BOTH
#undef SA_LAY_DT

// The entries of include/surya_amd.h over the bodies above. surya_op_lay_<op>(dtype, ...) keeps its contract of two dtypes (fp32 and bf16;
// anything else SA_ERR_UNSUPPORTED, which callers rely on); surya_op_lay_<op>_f16(...) is the same call on the fp16 instance.
int surya_op_lay_layernorm(int dtype, const void* x, const void* w, const void* b, void* y, const int32_t* perm, long rows, int rows_per_image, int C, float eps, int rows_per_image_out, void* stream) {
    return dtype == SA_DTYPE_F16 ? SA_ERR_UNSUPPORTED : lay_op_layernorm(dtype, x, w, b, y, perm, rows, rows_per_image, C, eps, rows_per_image_out, stream);
}
int surya_op_lay_layernorm_f16(const void* x, const void* w, const void* b, void* y, const int32_t* perm, long rows, int rows_per_image, int C, float eps, int rows_per_image_out, void* stream) { return lay_op_layernorm(SA_DTYPE_F16, x, w, b, y, perm, rows, rows_per_image, C, eps, rows_per_image_out, stream); }

int surya_op_lay_window_attn(int dtype, const void* qkv, const float* bias, void* out, long windows, int nh, int nkv, int nwx, int nwy, int shift, int ws, void* stream) {
    return dtype == SA_DTYPE_F16 ? SA_ERR_UNSUPPORTED : lay_op_window_attn(dtype, qkv, bias, out, windows, nh, nkv, nwx, nwy, shift, ws, stream);
}
int surya_op_lay_window_attn_f16(const void* qkv, const float* bias, void* out, long windows, int nh, int nkv, int nwx, int nwy, int shift, int ws, void* stream) { return lay_op_window_attn(SA_DTYPE_F16, qkv, bias, out, windows, nh, nkv, nwx, nwy, shift, ws, stream); }

int surya_op_lay_merge_ln(int dtype, const void* x, const void* w, const void* b, void* y, int B, int H, int W, int C, float eps, void* stream) {
    return dtype == SA_DTYPE_F16 ? SA_ERR_UNSUPPORTED : lay_op_merge_ln(dtype, x, w, b, y, B, H, W, C, eps, stream);
}
int surya_op_lay_merge_ln_f16(const void* x, const void* w, const void* b, void* y, int B, int H, int W, int C, float eps, void* stream) { return lay_op_merge_ln(SA_DTYPE_F16, x, w, b, y, B, H, W, C, eps, stream); }

int surya_op_lay_rows(int dtype, int kind, void* dst, const void* src, const int32_t* index, const int32_t* dims, void* stream) {
    return dtype == SA_DTYPE_F16 ? SA_ERR_UNSUPPORTED : lay_op_rows(dtype, kind, dst, src, index, dims, stream);
}
int surya_op_lay_rows_f16(int kind, void* dst, const void* src, const int32_t* index, const int32_t* dims, void* stream) { return lay_op_rows(SA_DTYPE_F16, kind, dst, src, index, dims, stream); }

int surya_op_lay_cross_attn(int dtype, int head_dim, const void* qpart, int S, int M, const void* kv, int n_images, const int32_t* item_map, void* out, float* scratch, void* vT, int nq, int nkv, int Lk, float scale, void* stream) {
    return dtype == SA_DTYPE_F16 ? SA_ERR_UNSUPPORTED : lay_op_cross_attn(dtype, head_dim, qpart, S, M, kv, n_images, item_map, out, scratch, vT, nq, nkv, Lk, scale, stream);
}
int surya_op_lay_cross_attn_f16(int head_dim, const void* qpart, int S, int M, const void* kv, int n_images, const int32_t* item_map, void* out, float* scratch, void* vT, int nq, int nkv, int Lk, float scale, void* stream) { return lay_op_cross_attn(SA_DTYPE_F16, head_dim, qpart, S, M, kv, n_images, item_map, out, scratch, vT, nq, nkv, Lk, scale, stream); }

int surya_op_lay_rmsnorm(int dtype, const void* x, const void* w, void* y, int rows, int C, float eps, void* stream) {
    return dtype == SA_DTYPE_F16 ? SA_ERR_UNSUPPORTED : lay_op_rmsnorm(dtype, x, w, y, rows, C, eps, stream);
}
int surya_op_lay_rmsnorm_f16(const void* x, const void* w, void* y, int rows, int C, float eps, void* stream) { return lay_op_rmsnorm(SA_DTYPE_F16, x, w, y, rows, C, eps, stream); }

int surya_op_lay_reduce_norm(int dtype, const float* part, int S, int M, const void* res, const void* bias, void* x_out, const void* w, void* y, int H, float eps, void* stream) {
    return dtype == SA_DTYPE_F16 ? SA_ERR_UNSUPPORTED : lay_op_reduce_norm(dtype, part, S, M, res, bias, x_out, w, y, H, eps, stream);
}
int surya_op_lay_reduce_norm_f16(const float* part, int S, int M, const void* res, const void* bias, void* x_out, const void* w, void* y, int H, float eps, void* stream) { return lay_op_reduce_norm(SA_DTYPE_F16, part, S, M, res, bias, x_out, w, y, H, eps, stream); }

int surya_op_lay_prefill_attn(int dtype, int head_dim, const void* qkv, void* out, void* kcache, void* vcache, const float* rope_cs, int B, int Tn, int nq, int nkv, int Tmax, float scale, void* stream) {
    return dtype == SA_DTYPE_F16 ? SA_ERR_UNSUPPORTED : lay_op_prefill_attn(dtype, head_dim, qkv, out, kcache, vcache, rope_cs, B, Tn, nq, nkv, Tmax, scale, stream);
}
int surya_op_lay_prefill_attn_f16(int head_dim, const void* qkv, void* out, void* kcache, void* vcache, const float* rope_cs, int B, int Tn, int nq, int nkv, int Tmax, float scale, void* stream) { return lay_op_prefill_attn(SA_DTYPE_F16, head_dim, qkv, out, kcache, vcache, rope_cs, B, Tn, nq, nkv, Tmax, scale, stream); }

int surya_op_lay_embed(int dtype, int family, const int32_t* tokens, const void* const* tabs, void* x, int rows, int Hd, int box_embed, int bbox_size, int vocab, int label_count, int category_count, int merge_count, void* stream) {
    return dtype == SA_DTYPE_F16 ? SA_ERR_UNSUPPORTED : lay_op_embed(dtype, family, tokens, tabs, x, rows, Hd, box_embed, bbox_size, vocab, label_count, category_count, merge_count, stream);
}
int surya_op_lay_embed_f16(int family, const int32_t* tokens, const void* const* tabs, void* x, int rows, int Hd, int box_embed, int bbox_size, int vocab, int label_count, int category_count, int merge_count, void* stream) { return lay_op_embed(SA_DTYPE_F16, family, tokens, tabs, x, rows, Hd, box_embed, bbox_size, vocab, label_count, category_count, merge_count, stream); }

int surya_op_lay_heads(int dtype, const void* x, long ldx, const void* fnorm_w, const void* ln_w, const void* ln_b, const void* lm_w, const void* bb_w, const void* bb_b, float* class_logits, float* bbox, int B, int Hd, int label_count, float rms_eps, float ln_eps, void* stream) {
    return dtype == SA_DTYPE_F16 ? SA_ERR_UNSUPPORTED : lay_op_heads(dtype, x, ldx, fnorm_w, ln_w, ln_b, lm_w, bb_w, bb_b, class_logits, bbox, B, Hd, label_count, rms_eps, ln_eps, stream);
}
int surya_op_lay_heads_f16(const void* x, long ldx, const void* fnorm_w, const void* ln_w, const void* ln_b, const void* lm_w, const void* bb_w, const void* bb_b, float* class_logits, float* bbox, int B, int Hd, int label_count, float rms_eps, float ln_eps, void* stream) { return lay_op_heads(SA_DTYPE_F16, x, ldx, fnorm_w, ln_w, ln_b, lm_w, bb_w, bb_b, class_logits, bbox, B, Hd, label_count, rms_eps, ln_eps, stream); }

int surya_op_gemm_geglu_f16(const void* X, long ldx, const void* W, long ldw, void* C, long ldc, int M, int N, int K, void* stream) {
    if (!X || !W || !C || N % 2) return SA_ERR_ARG;
    return sa::op_gemm_geglu(SA_DTYPE_F16, X, ldx, W, ldw, C, ldc, M, N, K, (hipStream_t)stream);
}

}  // extern "C"
