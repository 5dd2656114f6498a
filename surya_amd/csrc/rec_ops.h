// The recogniser's non-GEMM kernels alone (surya_op_rec_*, include/surya_amd.h): each entry packs its arguments into one of the plain
// structs below and runs rec_op<T>, which casts the pointers and calls the launcher RecModel<T> calls (kernels.h). float and bf16_t are
// instantiated in rec_model.hip, fp16_t in rec_model_f16.hip (op_rec_f16), as the engine is.
#pragma once
#include "kernels.h"
#include "beam.h"
#include "kv_fanout.h"
#include "kv_store.h"
#include "boost.h"

namespace sa {

struct RecRmsRowsOp { const void* x; long ldx; const void* w; void* y; long ldy; const int* src_row; int rows, C; float eps; };
struct RecRowsOp { int kind; void* dst; const void *src, *src2, *src3; const int *index, *index2, *index3; const int* dims; };
struct RecRopeTableOp { int kind; const int* pos_hw; const float* inv_freq; float* table; int n, d; };
struct RecRopeKvOp { void* qkv; const int *tok_slot, *tok_pos; const float* rope_cs; void *kc, *vc; int M, nq, nkv, D, Tmax; };
struct RecReduceOp { const float* part; int S, M; void* x; const void* w; void* y; int H; float eps; uint8_t *y8, *sy; int srows; };
struct RecEmbedOp {
    const void* table; const int *next_token, *active_slots, *kv_len; int Tmax; int* row_len; void* x; const void* w; void* y;
    int rows, H; float eps; uint8_t *y8, *sy; int srows;
};
struct RecKvForkOp { void *kc, *vc; const int *fork_src, *base, *len; int rows, layers, slots, nkv, Tmax, D; };
struct RecKvFanoutOp { void *kc, *vc; const int *fan_src, *fan_off, *fan_dst, *fan_len; int n_seqs, n_dst, layers, slots, nkv, Tmax, D; };
struct RecKvKeepOp {
    const void *kc, *vc; void *sk, *sv; const int *slot, *first, *len; int n, layers, slots, nkv, Tmax, D, cap; const void* x; const int* last_row;
    void* hid; int H, x_rows;
};
struct RecKvRestoreOp { void *kc, *vc; const void *sk, *sv; const int *first, *len, *fan_off, *fan_dst; int n, n_dst, layers, slots, nkv, Tmax, D, cap; };
enum { REC_OP_RMS_ROWS = 0, REC_OP_ROWS, REC_OP_ROPE_TABLE, REC_OP_ROPE_KV, REC_OP_REDUCE, REC_OP_EMBED, REC_OP_HEAD, REC_OP_KV_FORK, REC_OP_BOOST_HEAD,
       REC_OP_KV_FANOUT, REC_OP_KV_KEEP, REC_OP_KV_RESTORE };

template <typename T> constexpr bool rec_mx_ok() { return std::is_same<T, bf16_t>::value; }     // the MXFP8 copies exist beside bf16 only

template <typename T>
int rec_op(const RecRmsRowsOp& a, hipStream_t s) {
    if (!a.x || !a.w || !a.y || a.rows <= 0 || a.C <= 0) return SA_ERR_ARG;
    if (a.C % Ty<T>::V16 || a.ldx % Ty<T>::V16 || a.ldy % 4) return SA_ERR_SHAPE;
    return launch_rmsnorm<T>((const T*)a.x, a.ldx, (const T*)a.w, (T*)a.y, a.ldy, a.src_row, a.rows, a.C, a.eps, s);
}

template <typename T>
int rec_op(const RecRowsOp& a, hipStream_t s) {
    if (!a.dst || !a.src || !a.index || !a.dims) return SA_ERR_ARG;
    const int* d = a.dims;
    switch (a.kind) {
        case SA_REC_CONVERT_TILES:
            if (d[0] <= 0 || d[1] <= 0) return SA_ERR_ARG;
            return launch_convert_tiles<T>((const float*)a.src, (T*)a.dst, a.index, d[0], d[1], d[2], s);
        case SA_REC_SCATTER_IMAGE:
            if (!a.src2 || !a.src3 || !a.index2 || !a.index3 || d[0] <= 0 || d[1] <= 0) return SA_ERR_ARG;
            return launch_scatter_image<T>((const T*)a.src, (const T*)a.src2, (const T*)a.src3, a.index, a.index2, a.index3, (T*)a.dst, d[0], d[1], s);
        case SA_REC_SCATTER_ROWS:
            if (d[0] <= 0 || d[1] <= 0) return SA_ERR_ARG;
            return launch_scatter_rows<T>((const T*)a.src, a.index, (T*)a.dst, d[0], d[1], s);
        case SA_REC_EMBED_TOKENS:
            if (d[0] <= 0 || d[1] <= 0) return SA_ERR_ARG;
            return launch_embed_tokens<T>((const T*)a.src, a.index, (T*)a.dst, d[0], d[1], s);
    }
    return SA_ERR_ARG;
}

template <typename T>
int rec_op(const RecRopeTableOp& a, hipStream_t s) {
    if (!a.inv_freq || !a.table || a.n <= 0 || a.d <= 0) return SA_ERR_ARG;
    float2* tab = reinterpret_cast<float2*>(a.table);
    if (a.kind == SA_REC_ROPE_VISION) return a.pos_hw ? launch_rope_vision_table(a.pos_hw, a.inv_freq, tab, a.n, a.d, s) : SA_ERR_ARG;
    if (a.kind == SA_REC_ROPE_DECODER) return launch_rope_table<T>(a.inv_freq, tab, a.n, a.d, s);
    return SA_ERR_ARG;
}

template <typename T>
int rec_op(const RecRopeKvOp& a, hipStream_t s) {
    if (!a.qkv || !a.tok_slot || !a.tok_pos || !a.rope_cs || !a.kc || !a.vc || a.M <= 0 || a.Tmax <= 0) return SA_ERR_ARG;
    return launch_rope_kv_append<T>((T*)a.qkv, a.tok_slot, a.tok_pos, reinterpret_cast<const float2*>(a.rope_cs), (T*)a.kc, (T*)a.vc, a.M, a.nq,
                                    a.nkv, a.D, a.Tmax, s);
}

template <typename T>
int rec_op(const RecReduceOp& a, hipStream_t s) {
    if (!a.part || !a.x || a.S < 1 || a.S > 8 || a.M <= 0 || a.H <= 0 || (a.w && !a.y) || (a.y8 && (!a.sy || !a.w || a.srows < a.M))) return SA_ERR_ARG;
    if (a.y8 && !rec_mx_ok<T>()) return SA_ERR_UNSUPPORTED;
    if (a.y8 && a.H % 128) return SA_ERR_SHAPE;                  // whole 128-element K-tiles, as RecModel::set_mx_weights wants them
    return launch_reduce_norm<T>(a.part, a.S, a.M, (T*)a.x, (const T*)a.w, (T*)a.y, a.H, a.eps, a.y8, a.sy, a.srows, KvPrefetch(), s);
}

template <typename T>
int rec_op(const RecEmbedOp& a, hipStream_t s) {
    if (!a.table || !a.next_token || !a.active_slots || !a.kv_len || !a.row_len || !a.x || !a.w || !a.y || a.rows <= 0 || a.H <= 0 || a.Tmax <= 0 ||
        (a.y8 && (!a.sy || a.srows < a.rows)))
        return SA_ERR_ARG;
    if (a.y8 && !rec_mx_ok<T>()) return SA_ERR_UNSUPPORTED;
    return launch_decode_embed<T>((const T*)a.table, a.next_token, a.active_slots, a.kv_len, a.Tmax, a.row_len, (T*)a.x, (const T*)a.w, (T*)a.y, a.rows,
                                  a.H, a.eps, a.y8, a.sy, a.srows, a.y8 != nullptr, s);
}

template <typename T>
int rec_head_args(const surya_rec_head_args& a, HeadArgs<T>& h) {       // checked and cast: surya_op_rec_head and surya_op_rec_boost_head
    if (!a.part || !a.hidden || !a.wb || !a.bb || !a.row_slot || !a.out_token || !a.out_score || !a.out_bbox || !a.next_token || !a.kv_len ||
        a.rows <= 0 || a.tiles_n <= 0 || a.H <= 0)
        return SA_ERR_ARG;
    if (a.table && (!a.wnorm || !a.x || !a.y || !a.row_len || a.max_kv_len <= 0 || (a.y8 && (!a.sy || a.srows < a.rows)))) return SA_ERR_ARG;
    if (!a.table && a.y8) return SA_ERR_ARG;
    if (a.forced_table && (!a.forced_cursor || !a.flogit || a.forced_stride <= 0 || !a.greedy_token || !a.greedy_prob || !a.logprob || a.best_tot))
        return SA_ERR_ARG;                                       // (the engine refuses alternatives beside forced decoding)
    if (a.pat_tok_class && (!a.pat_next_state || !a.pat_state_mask || !a.pat_slot_state || !a.pat_slot_mask || a.pat_n_classes < 1 ||
                            a.pat_n_classes > SA_MAX_PATTERN_CLASSES || a.pat_vocab <= 0 || a.forced_table))
        return SA_ERR_ARG;                                       // (the engine refuses patterns beside forced decoding)
    if (a.y8 && !rec_mx_ok<T>()) return SA_ERR_UNSUPPORTED;
    if (a.H % 8 || (a.y8 && a.H % 128)) return SA_ERR_SHAPE;
    h = HeadArgs<T>{reinterpret_cast<const float4*>(a.part), a.tiles_n, a.rows, (const T*)a.hidden, a.H, (const T*)a.wb, (const T*)a.bb, a.row_slot,
                  a.eos_id, a.pad_id, a.bbox_size, a.out_token, a.out_score, a.out_bbox, a.next_token, a.kv_len, a.len_inc};
    h.table = (const T*)a.table; h.wnorm = (const T*)a.wnorm; h.x = (T*)a.x; h.y = (T*)a.y; h.row_len = a.row_len; h.Tmax = a.max_kv_len;
    h.eps = a.eps; h.y8 = a.y8; h.sy = a.sy; h.srows = a.srows;
    h.best_tot = reinterpret_cast<float2*>(a.best_tot);
    if (a.forced_table)
        h.fh = ForcedHead{a.forced_table, a.forced_cursor, a.flogit, a.forced_stride, a.greedy_token, a.greedy_prob, a.logprob};
    if (a.pat_tok_class)
        h.ph = PatternHead{a.pat_tok_class, a.pat_next_state, a.pat_state_mask, a.pat_n_classes, a.pat_vocab, a.pat_slot_state, a.pat_slot_mask};
    return SA_OK;
}

template <typename T>
int rec_op(const surya_rec_head_args& a, hipStream_t s) {
    HeadArgs<T> h;
    const int rc = rec_head_args<T>(a, h);
    return rc ? rc : launch_head<T>(h, a.y8 != nullptr, s);
}

template <typename T>
int rec_op(const surya_rec_boost_head_args& a, hipStream_t s) {
    if (!a.part_b || !a.slot_beta || !a.plain_token || !a.plain_prob || a.head.best_tot || a.head.forced_table || a.head.pat_tok_class) return SA_ERR_ARG;
    BoostHeadArgs<T> g;
    const int rc = rec_head_args<T>(a.head, g.h);
    if (rc) return rc;
    g.part_b = reinterpret_cast<const float4*>(a.part_b); g.slot_beta = a.slot_beta; g.plain_token = a.plain_token; g.plain_prob = a.plain_prob;
    return launch_boost_head<T>(g, a.head.y8 != nullptr, s);
}

template <typename T>
int rec_op(const RecKvForkOp& a, hipStream_t s) {
    if (a.rows < 0 || a.rows > a.slots) return SA_ERR_ARG;       // row r is slot r here (the engine passes its active list instead)
    return launch_kv_fork<T>((T*)a.kc, (T*)a.vc, nullptr, 1, a.fork_src, a.base, a.len, a.rows, a.layers, a.slots, a.nkv, a.Tmax, a.D, s);
}

template <typename T>
int rec_op(const RecKvFanoutOp& a, hipStream_t s) {
    return launch_kv_fanout<T>((T*)a.kc, (T*)a.vc, a.fan_src, a.fan_off, a.fan_dst, a.fan_len, a.n_seqs, a.n_dst, a.layers, a.slots, a.nkv, a.Tmax, a.D, s);
}

template <typename T>
int rec_op(const RecKvKeepOp& a, hipStream_t s) {
    return launch_kv_keep<T>((const T*)a.kc, (const T*)a.vc, (T*)a.sk, (T*)a.sv, a.slot, a.first, a.len, a.n, a.layers, a.slots, a.nkv, a.Tmax, a.D, a.cap,
                             (const T*)a.x, a.last_row, (T*)a.hid, a.H, a.x_rows, s);
}

template <typename T>
int rec_op(const RecKvRestoreOp& a, hipStream_t s) {
    return launch_kv_restore<T>((T*)a.kc, (T*)a.vc, (const T*)a.sk, (const T*)a.sv, a.first, a.len, a.fan_off, a.fan_dst, a.n, a.n_dst, a.layers, a.slots,
                                a.nkv, a.Tmax, a.D, a.cap, s);
}

template <typename T>
int rec_op_any(int op, const void* a, hipStream_t s) {
    switch (op) {
        case REC_OP_RMS_ROWS: return rec_op<T>(*static_cast<const RecRmsRowsOp*>(a), s);
        case REC_OP_ROWS: return rec_op<T>(*static_cast<const RecRowsOp*>(a), s);
        case REC_OP_ROPE_TABLE: return rec_op<T>(*static_cast<const RecRopeTableOp*>(a), s);
        case REC_OP_ROPE_KV: return rec_op<T>(*static_cast<const RecRopeKvOp*>(a), s);
        case REC_OP_REDUCE: return rec_op<T>(*static_cast<const RecReduceOp*>(a), s);
        case REC_OP_EMBED: return rec_op<T>(*static_cast<const RecEmbedOp*>(a), s);
        case REC_OP_HEAD: return rec_op<T>(*static_cast<const surya_rec_head_args*>(a), s);
        case REC_OP_KV_FORK: return rec_op<T>(*static_cast<const RecKvForkOp*>(a), s);
        case REC_OP_BOOST_HEAD: return rec_op<T>(*static_cast<const surya_rec_boost_head_args*>(a), s);
        case REC_OP_KV_FANOUT: return rec_op<T>(*static_cast<const RecKvFanoutOp*>(a), s);
        case REC_OP_KV_KEEP: return rec_op<T>(*static_cast<const RecKvKeepOp*>(a), s);
        case REC_OP_KV_RESTORE: return rec_op<T>(*static_cast<const RecKvRestoreOp*>(a), s);
    }
    return SA_ERR_ARG;
}

int op_rec_f16(int op, const void* args, hipStream_t s);       // rec_model_f16.hip: rec_op_any<fp16_t>

}  // namespace sa
