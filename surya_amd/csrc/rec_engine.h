// RecModel<T>: the recognition engine behind surya_rec_* (host-side planning + kernel sequencing), as a header so that each compute
// dtype is instantiated in a translation unit of its own: float and bf16_t in rec_model.hip, fp16_t in rec_model_f16.hip (a second
// 16-bit engine in one object would set the build's wall time). Everything here is a template, a plain struct or static.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <map>
#include <memory>
#include <set>
#include <vector>

#include "../../include/surya_amd.h"
#include "gemm.h"
#include "gemm_mx.h"
#include "kernels.h"
#include "decode_attn.h"
#include "decode_attn_kv8.h"
#include "kv_fanout.h"
#include "kv_store.h"
#include "attn_mfma.h"
#include "beam.h"
#include "automaton_core.h"
#include "lexicon.h"
#include "boost.h"

namespace sa {

// ------------------------------------------------------------------------------------------------- staging
struct Stager {   // pinned host arena mirrored by a device arena; one H2D copy per plan
    char* host = nullptr;
    char* dev = nullptr;
    size_t cap = 0, off = 0;
    hipEvent_t ev = nullptr;
    bool pending = false;
    int init(size_t bytes) {
        cap = bytes;
        SA_HIP(hipHostMalloc((void**)&host, cap, hipHostMallocDefault));
        SA_HIP(hipMalloc((void**)&dev, cap));
        SA_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        return SA_OK;
    }
    void destroy() {
        if (host) (void)hipHostFree(host);
        if (dev) (void)hipFree(dev);
        if (ev) (void)hipEventDestroy(ev);
        host = dev = nullptr; ev = nullptr;
    }
    void begin() {
        if (pending) { (void)hipEventSynchronize(ev); pending = false; }
        off = 0;
    }
    template <typename U> U* put(const U* src, size_t n) {   // returns the DEVICE address
        size_t bytes = n * sizeof(U);
        size_t o = (off + 255) & ~(size_t)255;
        if (o + bytes > cap) return nullptr;
        if (bytes) memcpy(host + o, src, bytes);
        off = o + bytes;
        return reinterpret_cast<U*>(dev + o);
    }
    template <typename U> U* put(const std::vector<U>& v) { return put(v.data(), v.size()); }
    int flush(hipStream_t s) {
        if (off) {
            SA_HIP(hipMemcpyAsync(dev, host, off, hipMemcpyHostToDevice, s));
            SA_HIP(hipEventRecord(ev, s));
            pending = true;
        }
        return SA_OK;
    }
};

// -------------------------------------------------------------------------------------------------- arenas
static size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

struct Carve {   // offsets of consecutive 256-byte-aligned blocks of one arena; `off` ends up as the arena's size
    size_t off = 0;
    size_t take(size_t bytes) { size_t o = off; off = align_up(off + bytes); return o; }
};

struct DevBlock {   // a zeroed device block and (host_bytes > 0) a pinned host block: both, or nothing
    char* dev = nullptr;
    char* host = nullptr;
    int alloc(size_t dev_bytes, size_t host_bytes) {
        char *d = nullptr, *h = nullptr;
        SA_HIP(hipMalloc((void**)&d, dev_bytes));
        int rc = host_bytes ? (int)hipHostMalloc((void**)&h, host_bytes, hipHostMallocDefault) : SA_OK;
        if (!rc) rc = (int)hipMemset(d, 0, dev_bytes);
        if (rc) { if (h) (void)hipHostFree(h); (void)hipFree(d); return rc; }
        dev = d; host = h;
        return SA_OK;
    }
    void release() {
        if (host) (void)hipHostFree(host);
        if (dev) (void)hipFree(dev);
        dev = host = nullptr;
    }
};

// A sparse automaton's tables (CSR: edge_off / edge_tok / edge_next, and a flag byte per state) in handle-owned memory sized by need,
// with their pinned staging copy: what lexicon-guided and boosted decoding each keep one of ("Sparse automata").
struct CsrDevice {
    DevBlock arena;                                      // device tables and the staging copy, same layout, [cap_states] / [cap_edges]
    int *edge_off = nullptr, *edge_tok = nullptr, *edge_next = nullptr;      // into arena.dev
    uint8_t* flags = nullptr;
    int cap_states = 0, cap_edges = 0;
    hipEvent_t ev = nullptr;                             // the staging copy is on the device
    bool pending = false;
    // Room for n_states / n_edges: powers of two from 1024, so a call's tables mostly fit the last call's. *moved = the tables are in a
    // new (zeroed) block and the old one is gone: captured steps hold stale addresses, and the feature is off until the next upload.
    // A failure changes nothing. Moving waits for the device: nothing in flight reads the old tables or their staging copy.
    int grow(int n_states, int n_edges, bool* moved) {
        *moved = false;
        if (n_states <= cap_states && n_edges <= cap_edges) return SA_OK;
        int cs = std::max(cap_states, 1024), ce = std::max(cap_edges, 1024);
        while (cs < n_states) cs *= 2;
        while (ce < n_edges) ce *= 2;
        Carve cv;
        const size_t o = cv.take(((size_t)cs + 1) * sizeof(int)), t = cv.take((size_t)ce * sizeof(int)), n = cv.take((size_t)ce * sizeof(int)),
                     f = cv.take((size_t)cs);
        DevBlock nb;
        int rc = nb.alloc(cv.off, cv.off);
        if (!rc && !ev) rc = (int)hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (!rc) rc = (int)hipDeviceSynchronize();
        if (rc) { nb.release(); return rc; }
        arena.release();
        arena = nb;
        pending = false;
        edge_off = reinterpret_cast<int*>(nb.dev + o);
        edge_tok = reinterpret_cast<int*>(nb.dev + t);
        edge_next = reinterpret_cast<int*>(nb.dev + n);
        flags = reinterpret_cast<uint8_t*>(nb.dev + f);
        cap_states = cs; cap_edges = ce;
        *moved = true;
        return SA_OK;
    }
    // Host tables -> staging copy -> device, in stream order, once the previous upload has left the staging copy. f == nullptr copies
    // no flags: they stay the zeros of the allocation.
    int upload(const int32_t* off, const int32_t* tok, const int32_t* next, const uint8_t* f, int n_states, int n_edges, hipStream_t s) {
        if (pending) { (void)hipEventSynchronize(ev); pending = false; }
        auto put = [&](void* dev, const void* src, size_t bytes) {
            char* h = arena.host + (static_cast<char*>(dev) - arena.dev);
            memcpy(h, src, bytes);
            return hipMemcpyAsync(dev, h, bytes, hipMemcpyHostToDevice, s);
        };
        SA_HIP(put(edge_off, off, ((size_t)n_states + 1) * sizeof(int)));
        if (n_edges) {
            SA_HIP(put(edge_tok, tok, (size_t)n_edges * sizeof(int)));
            SA_HIP(put(edge_next, next, (size_t)n_edges * sizeof(int)));
        }
        if (f) SA_HIP(put(flags, f, (size_t)n_states));
        SA_HIP(hipEventRecord(ev, s));
        pending = true;
        return SA_OK;
    }
    void release() {
        arena.release();
        if (ev) (void)hipEventDestroy(ev);
        ev = nullptr;
    }
};

// ------------------------------------------------------------------------------------------- step outputs
// One set of per-step outputs: per field a device array [SA_MAX_STEPS][max_slots][cell bytes] that the head kernels write at
// step * max_slots, and one pinned mirror that holds the fields one behind the other, each in the device array's order. Ring half r
// of a pipelined decode call starts at step r * SA_MAX_STEPS / 2. span() is the only place that turns (field, step) into addresses
// ("Step-output sets").
struct StepOutputs {
    static constexpr int MAX_FIELDS = 5;
    struct Field { const char* dev; size_t cell; };      // device array, bytes per (step, slot) cell
    struct Span { size_t host, dev, bytes; };            // byte offsets into the mirror and the device array, and the length
    Field f[MAX_FIELDS] = {};
    int n = 0;
    size_t slots = 0;                                    // max_slots
    char* host = nullptr;                                // the pinned mirror, host_bytes() long
    bool mirrored[2] = {false, false};                   // the last mirror-or-not decision on this ring half was "mirror"
    void add(const void* dev, size_t cell) { f[n++] = Field{static_cast<const char*>(dev), cell}; }
    size_t host_bytes() const { return span(n - 1, SA_MAX_STEPS, 0).host; }      // where the last field ends
    static int ring_step(int ring) { return ring * (SA_MAX_STEPS / 2); }
    // Field k starts at (the widths of the fields before it) * SA_MAX_STEPS * max_slots; inside a field a step is `slots` cells.
    Span span(int k, int step, int n_steps) const {
        const size_t full = (size_t)SA_MAX_STEPS * slots, off = (size_t)step * slots;
        size_t before = 0;
        for (int j = 0; j < k; ++j) before += f[j].cell;
        return Span{full * before + off * f[k].cell, off * f[k].cell, (size_t)n_steps * slots * f[k].cell};
    }
    // Async copies of steps [step, step + n_steps) to the mirror, one per field in field order (none for n_steps == 0).
    int copy(int step, int n_steps, hipStream_t s) const {
        for (int k = 0; k < n && n_steps; ++k) {
            const Span p = span(k, step, n_steps);
            SA_HIP(hipMemcpyAsync(host + p.host, f[k].dev + p.dev, p.bytes, hipMemcpyDeviceToHost, s));
        }
        return SA_OK;
    }
    int mirror(int ring, int n_steps, hipStream_t s) {   // the ring half's first n_steps steps
        mirrored[ring] = true;
        return copy(ring_step(ring), n_steps, s);
    }
    // The ring half's first n_steps steps out of the mirror (the caller has waited for the copies).
    void wait(int ring, int n_steps, void* const* dst) const {
        for (int k = 0; k < n; ++k) {
            const Span p = span(k, ring_step(ring), n_steps);
            memcpy(dst[k], host + p.host, p.bytes);
        }
    }
    // Steps [0, n_steps), synchronously.
    int read(int n_steps, void* const* dst, hipStream_t s) const {
        const int rc = copy(0, n_steps, s);
        if (rc) return rc;
        SA_HIP(hipStreamSynchronize(s));
        wait(0, n_steps, dst);
        return SA_OK;
    }
};

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

static __global__ void set_slot_state_kernel(const int* slots, const int* lens, int* kv_len, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) kv_len[slots[i]] = lens[i];
}
static __global__ void set_next_tokens_kernel(const int* slots, const int* toks, int* next_token, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) next_token[slots[i]] = toks[i];
}

// --------------------------------------------------------------------------------------------------- model
// The step-output sets of an engine, in the order decode_async mirrors them; the fields of each in the order of its surya_rec_read_* /
// surya_rec_wait_* arguments (RecModel::init names them).
enum StepSet { STEPS_BASE = 0, STEPS_ALTS, STEPS_BEAM, STEPS_FORCED, STEPS_BOOST, STEPS_SETS };

struct RecBase {
    virtual ~RecBase() {}
    virtual int prefill(const float*, const int32_t*, int, const int32_t*, const int32_t*, const int32_t*, int, hipStream_t) = 0;
    virtual int prefill_shared(const float*, const int32_t*, int, const int32_t*, const int32_t*, const int32_t*, const int32_t*, int, hipStream_t) = 0;
    virtual int reserve_prompts(int, hipStream_t) = 0;
    virtual int prefill_keep(const float*, const int32_t*, int, const int32_t*, const int32_t*, const int32_t*, int, const int32_t*, hipStream_t) = 0;
    virtual int restore(const int32_t*, const int32_t*, const int32_t*, int, hipStream_t) = 0;
    virtual int drop_prompts(const int32_t*, int) = 0;
    virtual int prompt_store_info(int32_t*, int32_t*) = 0;
    virtual int set_active(const int32_t*, int, hipStream_t) = 0;
    virtual int encode_ahead(const float*, const int32_t*, int, hipStream_t) = 0;
    virtual int decode(int, hipStream_t) = 0;
    virtual int decode_async(int, int, hipStream_t) = 0;
    virtual int read_steps(StepSet, int n_steps, std::initializer_list<void*> dst, hipStream_t) = 0;     // dst: one pointer per field of the set
    virtual int wait_steps(StepSet, int n_steps, int ring, std::initializer_list<void*> dst) = 0;
    virtual int encode_only(const float*, const int32_t*, int, void*, hipStream_t) = 0;
    virtual int copy_last_logits(float*, int, int*, hipStream_t) = 0;
    virtual int copy_kv_rows(int, int, void*, void*, hipStream_t) = 0;
    virtual int set_next_tokens(const int32_t*, const int32_t*, int, hipStream_t) = 0;
    virtual int set_mx_weights(const void* const*, int) = 0;
    virtual int set_kv_fp8(int) = 0;
    virtual int set_token_masks(const uint32_t*, int, hipStream_t) = 0;
    virtual int set_slot_masks(const int32_t*, const int32_t*, int, hipStream_t) = 0;
    virtual int set_alternatives(int) = 0;
    virtual int set_forced(int) = 0;
    virtual int set_forced_tokens(const int32_t*, const int32_t*, const int32_t*, int, hipStream_t) = 0;
    virtual int set_beam(int, int) = 0;
    virtual int set_patterns(const uint8_t*, const uint16_t*, const uint8_t*, int, int, hipStream_t) = 0;
    virtual int set_slot_patterns(const int32_t*, const int32_t*, int, hipStream_t) = 0;
    virtual int copy_slot_states(int32_t*, hipStream_t) = 0;
    virtual int set_lexicon(const int32_t*, const int32_t*, const int32_t*, const uint8_t*, int, int, int, hipStream_t) = 0;
    virtual int set_slot_lexicon(const int32_t*, const int32_t*, int, hipStream_t) = 0;
    virtual int copy_lexicon_states(int32_t*, hipStream_t) = 0;
    virtual int set_boost(const int32_t*, const int32_t*, const int32_t*, int, int, int, int, hipStream_t) = 0;
    virtual int set_slot_boost(const int32_t*, const int32_t*, const float*, int, hipStream_t) = 0;
    virtual int copy_boost_states(int32_t*, hipStream_t) = 0;
};

// surya_rec_set_forced_tokens: workgroup i writes the whole table row of slots[i] -- its ids, then -1 -- and sets the slot's cursor to 0
static __global__ __launch_bounds__(256) void set_forced_tokens_kernel(const int* slots, const int* tokens, const int* offsets, int* table,
                                                                       int* cursor, int stride) {
    const int i = blockIdx.x, slot = slots[i], a = offsets[i], len = offsets[i + 1] - a;
    for (int j = threadIdx.x; j < stride; j += 256) table[(long)slot * stride + j] = j < len ? tokens[a + j] : -1;
    if (threadIdx.x == 0) cursor[slot] = 0;
}

static __global__ void set_slot_masks_kernel(const int* slots, const int* ids, int* slot_mask, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) slot_mask[slots[i]] = ids[i];
}

// surya_rec_set_slot_patterns (states != nullptr): slot_state = the start state, and where it is >= 0 the slot's mask id = that state's row.
// surya_rec_set_slot_masks on a handle with pattern memory (states == nullptr): the named slots follow no automaton any more.
static __global__ void set_slot_patterns_kernel(const int* slots, const int* states, const uint8_t* state_mask, int* slot_state, int* slot_mask,
                                                int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int slot = slots[i], st = states ? states[i] : -1;
    slot_state[slot] = st;
    if (st >= 0) slot_mask[slot] = state_mask[st];
}

template <int I> using HeadEpi = std::integral_constant<int, I>;      // compile-time index into a weight format's lm_head epilogues (heads())

template <typename T>
struct RecModel : RecBase {
    surya_rec_config c;
    std::vector<const void*> w;
    char* arena = nullptr;
    size_t arena_bytes = 0;
    Stager st, st_small, st_enc;                         // st_enc: plans of the look-ahead encoder (its own stream)
    hipStream_t estream = nullptr;                       // low-priority stream of the look-ahead encoder
    hipEvent_t ev_ahead_in = nullptr, ev_ahead_done = nullptr, ev_ahead_free = nullptr;
    T* emb_ahead = nullptr;                              // [max_prefill_tokens][dec_hidden] image embeddings encoded ahead
    long ahead_tokens = 0, ahead_consumed = 0;
    bool ahead_free_recorded = false;
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
    int *kv_len, *next_token, *active_dev, *row_len;
    int* out_token; float* out_score; int* out_bbox;     // [SA_MAX_STEPS][max_slots] (bbox x6)
    size_t out_bytes = 0;
    StepOutputs outs[STEPS_SETS];                        // what decode_async mirrors and read_steps / wait_steps return (StepOutputs above)
    int n_active = 0;
    int last_rows = 0;
    bool last_heads_mx = false;                          // the last heads() call ran the MXFP8 lm_head (test hook below)
    // hipGraph replay of decode steps: a step is ~113 short launches; captured once per (active rows, steps) and replayed
    // from an internal stream (capture is not allowed on the legacy default stream torch hands us).
    hipStream_t gstream = nullptr;
    hipEvent_t gev_in = nullptr, gev_out = nullptr;
    hipEvent_t ev_ring[2] = {nullptr, nullptr};          // outputs of ring half r are in the pinned mirror
    std::map<long, hipGraphExec_t> graphs;
    std::set<long> seen_keys;
    bool use_graph = true;
    int graph_epoch = 0;                                 // tuning_epoch() the cached graphs were captured under
    // Host-side upper bounds of kv_len (set at prefill, +1 per decode step of an active slot): they only pick the decode-attention
    // variant -- two K/V tile buffers once some active context exceeds one 128-key tile -- and never enter a result.
    std::vector<int> h_len, h_active;
    int ctx_bound = 0;                                   // cached keys + the new one, max over the active slots, of the step being enqueued
                                                         // (not consulted with hipGraph replay on: a captured step must not depend on host state)
    // MXFP8 decode weights (surya_rec_set_mx_weights; gemm_mx.h): e4m3 copies + e8m0 block scales of the decoder projections
    // and lm_head, used by the decode steps only (prefill keeps the bf16 weights), and MXFP8 twins of the four decode-step
    // activation buffers, written by the kernels that produce the bf16 ones.
    std::vector<const uint8_t*> mxw;
    DevBlock mx_arena;
    // FP8 KV cache of the decode steps (surya_rec_set_kv_fp8; decode_attn_kv8.h). Prefill keeps writing (and attending over) the
    // bf16 cache and quantises the prompt rows into these arrays; the decode steps read and append only here.
    DevBlock kv8_arena;
    uint8_t *k8c = nullptr, *v8tc = nullptr;     // [layer][slot][kvh][Tmax][D], [layer][slot][kvh][D][Tmax8]
    float *ksc8 = nullptr, *vsc8 = nullptr;      // [layer][slot][kvh][Tmax8]
    bool kv8 = false;
    int tmax8() const { return kv8_tmax(c.max_kv_len); }
    uint8_t *dh8 = nullptr, *sdh = nullptr, *dattn8 = nullptr, *sattn = nullptr, *dmlp8 = nullptr, *smlp = nullptr, *dlast8 = nullptr,
            *slast = nullptr;
    static constexpr bool MX_OK = std::is_same<T, bf16_t>::value;     // MXFP8 weights / activations exist beside the bf16 engine only
    bool mx() const { return MX_OK && !mxw.empty(); }
    // Allowed-character sets (surya_rec_set_token_masks / surya_rec_set_slot_masks; TokenMask in gemm.h): a table of SA_MAX_TOKEN_MASKS
    // bit rows over the vocabulary and one row id per slot, at addresses that never change once allocated -- captured decode steps hold
    // the pointers, the contents follow the calls in stream order. n_token_masks == 0: the unmasked lm_head kernels, as ever.
    char* mask_arena = nullptr;
    uint32_t* mask_table = nullptr;                      // [SA_MAX_TOKEN_MASKS][mask_words()]
    int* slot_mask = nullptr;                            // [max_slots], -1 = unconstrained
    Stager st_mask;
    int n_token_masks = 0;
    int mask_words() const { return cdiv(c.vocab, 32); }
    TokenMask token_mask(const int* d_row_slot) const { return TokenMask{mask_table, slot_mask, d_row_slot, mask_words()}; }
    // Alternatives (surya_rec_set_alternatives): per-tile candidates of the lm_head's *_TOPK epilogue, the head's (max, total) per slot and
    // the [SA_MAX_STEPS][max_slots][SA_MAX_ALTERNATIVES] outputs with their pinned mirror, allocated on the first switch-on at addresses
    // that never change afterwards. alts == false: the lm_head and head launches are the ones of a handle without this entry.
    DevBlock alt_arena;
    float2* alt_part = nullptr;                          // [max_slots][cdiv(vocab, 64)][4]: 64 columns is the narrowest lm_head tile
    float2* best_tot = nullptr;                          // [max_slots]
    int* alt_token = nullptr; float* alt_prob = nullptr; // [SA_MAX_STEPS][max_slots][4]
    bool alts = false;
    // Forced decoding (surya_rec_set_forced): the id table [max_slots][SA_MAX_FORCED_TOKENS] (-1 = free-running), a cursor per slot, the
    // forced logit per lm_head row, the [SA_MAX_STEPS][max_slots] outputs and their pinned mirror, allocated on the first switch-on at
    // addresses that never change afterwards. forcing == false: the lm_head and head launches are the ones of a handle without this entry.
    DevBlock forced_arena;
    int* forced_table = nullptr; int* forced_cursor = nullptr; float* flogit = nullptr;
    int* greedy_token = nullptr; float* greedy_prob = nullptr; float* forced_logprob = nullptr;   // [SA_MAX_STEPS][max_slots]
    Stager st_forced;
    bool forcing = false;
    ForcedCols forced_cols(const int* d_row_slot) const { return ForcedCols{forced_table, forced_cursor, d_row_slot, SA_MAX_FORCED_TOKENS, flogit}; }
    // Beam search (surya_rec_set_beam; beam.h, beam_core.h): per slot the beam's cumulative score, finished flag, its group's prompt length
    // and the fork plan of the step (source slot, first row, row count); the five [SA_MAX_STEPS][max_slots] outputs and their pinned mirror,
    // allocated on the first switch-on at addresses that never change afterwards. beam == 0: every launch is the one of a handle without
    // this entry. beam > 0: the lm_head runs its *_TOPK epilogue whatever `alts` says, and the head never fuses the next step's embedding.
    DevBlock beam_arena;
    float* beam_score = nullptr; int *beam_fin = nullptr, *beam_prompt = nullptr, *fork_src = nullptr, *fork_base = nullptr, *fork_len = nullptr;   // [max_slots]
    int *beam_token = nullptr, *beam_parent = nullptr, *beam_rank = nullptr; float *beam_prob = nullptr, *beam_logp = nullptr;
    int beam = 0, beam_nop = -1;
    // Pattern-guided decoding (surya_rec_set_patterns; PatternHead in kernels.h): the automaton's three tables at their largest size and a
    // state per slot, allocated on the first call at addresses that never change afterwards -- captured decode steps hold the pointers,
    // the contents follow the calls in stream order. pat_states == 0: the head launches are the ones of a handle without this entry.
    char* pat_arena = nullptr;
    uint8_t* pat_tok_class = nullptr;                    // [vocab]
    uint16_t* pat_next_state = nullptr;                  // [SA_MAX_PATTERN_STATES][SA_MAX_PATTERN_CLASSES]: rows always SA_MAX_PATTERN_CLASSES
                                                         // apart, so a captured head launch holds for tables of any class count
    uint8_t* pat_state_mask = nullptr;                   // [SA_MAX_PATTERN_STATES]
    int* slot_state = nullptr;                           // [max_slots], -1 = no pattern
    Stager st_pat;
    int pat_states = 0, pat_classes = 0;
    // Lexicon-guided decoding (surya_rec_set_lexicon; lexicon.h): the tables and a state per slot, allocated on the first call at an
    // address that never changes. Switching on or off drops captured steps. Slot s owns row SA_MAX_TOKEN_MASKS + s of the mask table; those
    // max_slots rows exist only on a handle that has seen a lexicon (mask_dyn_rows: the first set_lexicon moves the mask arena into a
    // larger block, at the one moment at which every captured step is dropped anyway; from then on its addresses never move again).
    // lex_states == 0: the handle launches exactly what a handle without this entry launches.
    CsrDevice lex;
    int* slot_lex_state = nullptr;                       // [max_slots], -1 = no lexicon
    Stager st_lex;                                       // slots and start states of set_slot_lexicon
    bool mask_dyn_rows = false;
    int lex_states = 0, lex_nop = -1;
    LexiconArgs csr_args(const CsrDevice& t, int* slot_st, int nop) const {
        return LexiconArgs{t.edge_off, t.edge_tok, t.edge_next, t.flags, mask_table, mask_words(), SA_MAX_TOKEN_MASKS, slot_st, slot_mask,
                           c.vocab, c.eos_token_id, c.pad_token_id, nop};
    }
    LexiconArgs lex_args() const { return csr_args(lex, slot_lex_state, lex_nop); }
    // Boosted decoding (surya_rec_set_boost; boost.h): the tables; state, root and beta per slot, the second lm_head partial buffer
    // (record B) and the STEPS_BOOST outputs with their pinned mirror, allocated on the first call at addresses that never change. A
    // boosted slot owns the mask-table row a lexicon slot would. bst_states == 0: the handle launches what one without this entry does.
    CsrDevice bst;                                       // (state_flags: the zeros of the allocation, never uploaded)
    DevBlock bst_slots;                                  // per-slot state / root / beta, record B's partials, the outputs and their mirror
    int *slot_bst_state = nullptr, *slot_bst_root = nullptr; float* slot_bst_beta = nullptr;     // [max_slots]: -1, -1, +inf = not boosted
    float4* amax_b = nullptr;                            // as amax
    int* plain_token = nullptr; float* plain_prob = nullptr;     // [SA_MAX_STEPS][max_slots]
    Stager st_bst;                                       // slots, roots and betas of set_slot_boost
    int bst_states = 0, bst_out = 0, bst_word_row = 0;
    BoostArgs bst_args() const {
        return BoostArgs{TotalOps{slot_bst_root, slot_bst_beta, bst_out, bst_word_row}, csr_args(bst, slot_bst_state, -1)};
    }
    // The slot list of a set_slot_* call: 1 <= n <= max_slots entries, every slot in range and named once (which value would win is a
    // race in the scatter), and also(i), the call's own check of entry i, holds. SA_OK or SA_ERR_ARG.
    template <typename F>
    int check_slots(const int32_t* slots, int n, F&& also) const {
        std::vector<char> seen(c.max_slots, 0);
        for (int i = 0; i < n; ++i) {
            if (slots[i] < 0 || slots[i] >= c.max_slots || seen[slots[i]] || !also(i)) return SA_ERR_ARG;
            seen[slots[i]] = 1;
        }
        return SA_OK;
    }
    int copy_states(int32_t* dst, const int* states, hipStream_t s) const {      // the three copy_*_states
        if (!states) return SA_ERR_STATE;
        SA_HIP(hipMemcpyAsync(dst, states, (size_t)c.max_slots * sizeof(int), hipMemcpyDeviceToDevice, s));
        return SA_OK;
    }
    bool topk() const { return alts || beam > 0; }       // the lm_head collects candidates and topk_combine_kernel runs
    // Which step-output sets the kernels write right now: decode_async mirrors these, read_steps / wait_steps refuse the others.
    bool steps_on(StepSet k) const { return k == STEPS_BASE || (k == STEPS_ALTS && topk()) || (k == STEPS_BEAM && beam > 0) || (k == STEPS_FORCED && forcing) || (k == STEPS_BOOST && bst_states > 0); }
    // The modes that cannot be on together, and why; every setter asks excluded() before it switches its own mode on.
    enum Mode { M_MASKS, M_ALTS, M_FORCED, M_BEAM, M_KV8, M_MX, M_PATTERNS, M_LEXICON, M_BOOST, MODES };
    bool mode_on(int m) const { const bool on[MODES] = {n_token_masks > 0, alts, forcing, beam > 0, kv8, mx(), pat_states > 0, lex_states > 0, bst_states > 0}; return on[m]; }
    bool excluded(int m) const {
        static constexpr int pairs[14][2] = {{M_FORCED, M_MASKS},      // forced decoding runs the unmasked partial
                                            {M_FORCED, M_ALTS},       // ... which collects no candidates
                                            {M_FORCED, M_BEAM},
                                            {M_BEAM, M_KV8},          // the KV fork copies the bf16 / fp16 / fp32 caches only
                                            {M_BEAM, M_MX},          // (beam search on the fp8 decode paths is out of scope: DESIGN.md 4l)
                                            {M_FORCED, M_PATTERNS},   // patterns move mask ids, and forced decoding reads no mask
                                            {M_BEAM, M_PATTERNS},     // a surviving beam would have to inherit its PARENT's state through
                                                                      // beam_select_kernel's choice: left out for now
                                            {M_FORCED, M_LEXICON},    // as patterns: forced decoding reads no mask,
                                            {M_BEAM, M_LEXICON},      // and a surviving beam would inherit its parent's state AND row (4o)
                                            {M_BOOST, M_ALTS},        // boosting runs the masked and the plain greedy epilogue, alternatives,
                                            {M_BOOST, M_BEAM},        // beam search and forced decoding run others (4p)
                                            {M_BOOST, M_FORCED},
                                            {M_BOOST, M_PATTERNS},    // their heads and rows would have to be combined with the boost's:
                                            {M_BOOST, M_LEXICON}};    // the follow-up (4p)
        for (auto& p : pairs)
            if ((p[0] == m && mode_on(p[1])) || (p[1] == m && mode_on(p[0]))) return true;
        return false;
    }
    const uint8_t* MXW(int l, int k) const { return mxw[(size_t)l * SA_MX_COUNT + k]; }
    const uint8_t* MXG(int k) const { return mxw[(size_t)c.dec_layers * SA_MX_COUNT + k]; }

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
            char* b = m->arena;
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
        SA_HIP(hipMalloc((void**)&arena, arena_bytes));
        poison_arena(arena, arena_bytes);
        layout(c, this);
        {
            const int rc = launch_rope_table<T>(reinterpret_cast<const float*>(w[SA_RW_DEC_INVFREQ]), rope_cs, c.max_kv_len, c.dec_head_dim / 2, 0);
            if (rc) return rc;
        }
        SA_HIP(hipMemset(kv_len, 0, c.max_slots * sizeof(int)));
        SA_HIP(hipMemset(next_token, 0, c.max_slots * sizeof(int)));
        SA_HIP(hipMemset(out_token, 0, out_bytes));
        for (auto& o : outs) o.slots = c.max_slots;
        StepOutputs& base = outs[STEPS_BASE];              // always on: a ring half counts as mirrored from the start
        base.add(out_token, 4); base.add(out_score, 4); base.add(out_bbox, 24);
        base.mirrored[0] = base.mirrored[1] = true;
        SA_HIP(hipHostMalloc((void**)&base.host, base.host_bytes(), hipHostMallocDefault));     // (the other sets' mirrors come with their arenas)
        const size_t Pm = c.max_patches, Tm = std::max(c.max_prefill_tokens, c.max_slots);
        int rc = st.init((Pm * 8 + Tm * 8 + (size_t)c.max_slots * 64) * sizeof(int) + (1 << 20));
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
    ~RecModel() override {
        for (DevBlock* b : {&mx_arena, &kv8_arena, &alt_arena, &beam_arena, &forced_arena, &store}) b->release();
        if (mask_arena) (void)hipFree(mask_arena);
        if (pat_arena) (void)hipFree(pat_arena);
        lex.release(); bst.release(); bst_slots.release();
        if (slot_lex_state) (void)hipFree(slot_lex_state);
        st_mask.destroy(); st_forced.destroy(); st_pat.destroy(); st_lex.destroy(); st_bst.destroy();
        for (auto& kv : graphs) (void)hipGraphExecDestroy(kv.second);
        if (gstream) (void)hipStreamDestroy(gstream);
        if (gev_in) (void)hipEventDestroy(gev_in);
        if (gev_out) (void)hipEventDestroy(gev_out);
        for (auto e : ev_ring) if (e) (void)hipEventDestroy(e);
        st.destroy(); st_small.destroy(); st_enc.destroy();
        if (estream) (void)hipStreamDestroy(estream);
        for (hipEvent_t e : {ev_ahead_in, ev_ahead_done, ev_ahead_free}) if (e) (void)hipEventDestroy(e);
        if (arena) (void)hipFree(arena);
        if (outs[STEPS_BASE].host) (void)hipHostFree(outs[STEPS_BASE].host);
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
    // Activation scale tensors are K-tile-major with max_slots rows per K-tile ([K / 128][max_slots][4]); a row range of the
    // batch is a pointer offset of 4 bytes per row.
    int splitk_gemm_mx(const uint8_t* X, const uint8_t* SX, long ldx, const uint8_t* Wq, const uint8_t* SW, int M, int N, int K,
                       float* part_, int* S, hipStream_t s) {
        MxArgs a{X, ldx, SX, Wq, (long)K, SW, M, N, K, (long)c.max_slots, (long)N};
        a.part = part_;
        int rc = launch_gemm_mx_splitk(a, s);
        *S = a.splitk;
        return rc;
    }

    // FP8 KV cache for the decode steps (bf16 model only). Takes effect for lines prefilled AFTER the call: switch while no line
    // is in flight.
    // Captured decode steps hold launch arguments AND kernel choices: any mode change (fp8 KV cache, MXFP8 weights, a tuning knob)
    // must drop them, or a replay would run the other attention kernel on a cache the new shapes no longer append to.
    void drop_graphs() {
        for (auto& kv : graphs) (void)hipGraphExecDestroy(kv.second);
        graphs.clear(); seen_keys.clear();
    }
    int set_kv_fp8(int on) override {
        if constexpr (!std::is_same<T, bf16_t>::value) return on ? SA_ERR_UNSUPPORTED : SA_OK;
        if (on && excluded(M_KV8)) return SA_ERR_STATE;
        if ((on != 0) != kv8) drop_graphs();
        if (!on) { kv8 = false; return SA_OK; }
        const int d = c.dec_head_dim;
        if (d != 128 && d != 64 && d != 32) return SA_ERR_UNSUPPORTED;
        if (c.dec_heads / c.dec_kv_heads > 8) return SA_ERR_UNSUPPORTED;
        if (!kv8_arena.dev) {
            const size_t rows = (size_t)c.dec_layers * c.max_slots * c.dec_kv_heads, T8 = tmax8();
            Carve cv;
            const size_t o_k = cv.take(rows * c.max_kv_len * d), o_v = cv.take(rows * d * T8), o_ks = cv.take(rows * T8 * 4), o_vs = cv.take(rows * T8 * 4);
            const int rc = kv8_arena.alloc(cv.off, 0);      // zeroed: finite bytes and scales everywhere, masked key columns multiply P = 0
            if (rc) return rc;
            char* b = kv8_arena.dev;
            k8c = (uint8_t*)(b + o_k); v8tc = (uint8_t*)(b + o_v);
            ksc8 = (float*)(b + o_ks); vsc8 = (float*)(b + o_vs);
            SA_HIP(hipDeviceSynchronize());
        }
        kv8 = true;
        return SA_OK;
    }

    // The mask table of the lm_head's greedy epilogues. Every row needs an allowed id inside the vocabulary: a row without one would
    // make the head emit the "no column" index 0x7fffffff and the next step embed it. Replacing the table sets every slot back to -1 (the
    // ids named rows of the old table). Switching between the masked and the unmasked kernels drops captured steps, as set_kv_fp8 does.
    int set_token_masks(const uint32_t* masks, int n, hipStream_t s) override {
        if (n < 0 || n > SA_MAX_TOKEN_MASKS || (n > 0 && !masks)) return SA_ERR_ARG;
        if (n > 0 && excluded(M_MASKS)) return SA_ERR_STATE;
        const int words = mask_words();
        for (int i = 0; i < n; ++i) {
            bool any = false;
            for (int wd = 0; wd < words && !any; ++wd) {
                const int left = c.vocab - wd * 32;                     // bits of the last word past the vocabulary do not count
                any = (masks[(size_t)i * words + wd] & (left >= 32 ? 0xffffffffu : ((1u << left) - 1u))) != 0;
            }
            if (!any) return SA_ERR_ARG;
        }
        if (n == 0) {
            if (n_token_masks > 0) drop_graphs();
            n_token_masks = 0;
            return automata_off(s);
        }
        const size_t table_bytes = (size_t)SA_MAX_TOKEN_MASKS * words * sizeof(uint32_t);
        if (!mask_arena) {                                  // first table: memory and staging, or nothing (a failure leaves the handle as it was)
            Carve cv;
            const size_t o_slot = cv.take((size_t)c.max_slots * sizeof(int)), o_table = cv.take(table_bytes);   // (grow_mask_arena: same layout)
            char* mem = nullptr;
            SA_HIP(hipMalloc((void**)&mem, cv.off));
            int rc = st_mask.init(table_bytes + (size_t)c.max_slots * 2 * sizeof(int) + 4096);
            if (!rc) rc = (int)hipMemsetAsync(mem, 0xff, cv.off, s);      // every slot -1, every column allowed
            if (rc) { st_mask.destroy(); st_mask = Stager(); (void)hipFree(mem); return rc; }
            mask_arena = mem;
            slot_mask = reinterpret_cast<int*>(mask_arena + o_slot);
            mask_table = reinterpret_cast<uint32_t*>(mask_arena + o_table);
        }
        st_mask.begin();
        const uint32_t* d = st_mask.put(masks, (size_t)n * words);
        if (!d) return SA_ERR_NOMEM;
        int rc = st_mask.flush(s);
        if (rc) return rc;
        SA_HIP(hipMemsetAsync(slot_mask, 0xff, (size_t)c.max_slots * sizeof(int), s));
        SA_HIP(hipMemcpyAsync(mask_table, d, (size_t)n * words * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
        if (n_token_masks == 0) drop_graphs();              // only once the new table is on its way: a refused call changes nothing
        n_token_masks = n;
        return automata_off(s);                             // the state -> row map named rows of the old table; every slot's id is -1 again
    }
    // Mask ids of the slots about to be prefilled (-1 = unconstrained); a slot keeps its id until it is set again.
    int set_slot_masks(const int32_t* slots, const int32_t* ids, int n, hipStream_t s) override {
        if (n <= 0) return n < 0 ? SA_ERR_ARG : SA_OK;
        if (n > c.max_slots) return SA_ERR_ARG;
        if (n_token_masks == 0) return SA_ERR_STATE;
        if (check_slots(slots, n, [&](int i) { return ids[i] >= -1 && ids[i] < n_token_masks; })) return SA_ERR_ARG;
        st_mask.begin();
        const int* ds = st_mask.put(slots, n);
        const int* di = st_mask.put(ids, n);
        if (!di) return SA_ERR_NOMEM;
        int rc = st_mask.flush(s);
        if (rc) return rc;
        hipLaunchKernelGGL(set_slot_masks_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, ds, di, slot_mask, n);
        if (slot_state)                                     // a slot given a plain id follows no automaton any more (a reused slot would go on advancing)
            hipLaunchKernelGGL(set_slot_patterns_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, ds, (const int*)nullptr, pat_state_mask, slot_state,
                               slot_mask, n);
        if ((rc = (int)hipGetLastError())) return rc;
        if (slot_lex_state && (rc = launch_lexicon_start(lex_args(), ds, nullptr, n, s))) return rc;      // ... and rewrites no row any more
        if (slot_bst_state) return launch_boost_start(bst_args(), ds, nullptr, nullptr, n, s);            // ... and is not boosted any more
        return SA_OK;
    }
    int automata_off(hipStream_t s) {
        int rc = patterns_off(s);
        if (!rc) rc = lexicon_off(s);
        return rc ? rc : boost_off(s);
    }

    // The automaton of pattern-guided decoding. Every entry is checked against the counts and the current mask table before anything is
    // enqueued: the head reads next_state[state][class] and state_mask[state] unchecked. New tables set every slot's state back to -1.
    // Switching between on and off drops captured steps, which hold the head's empty / filled PatternHead; new contents keep them.
    int set_patterns(const uint8_t* tok_class, const uint16_t* next_state, const uint8_t* state_mask, int n_states, int n_classes,
                     hipStream_t s) override {
        if (n_states < 0 || n_states > SA_MAX_PATTERN_STATES) return SA_ERR_ARG;
        if (n_states == 0) return patterns_off(s);
        if (n_classes < 1 || n_classes > SA_MAX_PATTERN_CLASSES || !tok_class || !next_state || !state_mask) return SA_ERR_ARG;
        if (n_token_masks == 0 || excluded(M_PATTERNS)) return SA_ERR_STATE;
        const size_t n_next = (size_t)n_states * n_classes;
        for (int v = 0; v < c.vocab; ++v)
            if (tok_class[v] >= n_classes) return SA_ERR_ARG;
        for (size_t i = 0; i < n_next; ++i)
            if (next_state[i] >= n_states) return SA_ERR_ARG;
        for (int i = 0; i < n_states; ++i)
            if (state_mask[i] >= n_token_masks) return SA_ERR_ARG;
        const size_t next_bytes = (size_t)SA_MAX_PATTERN_STATES * SA_MAX_PATTERN_CLASSES * sizeof(uint16_t), S = c.max_slots;
        if (!pat_arena) {                                   // first tables: memory and staging, or nothing (a failure leaves the handle as it was)
            Carve cv;
            const size_t o_slot = cv.take(S * sizeof(int)), o_cls = cv.take(c.vocab), o_mask = cv.take(SA_MAX_PATTERN_STATES),
                         o_next = cv.take(next_bytes);
            char* mem = nullptr;
            Stager st;
            SA_HIP(hipMalloc((void**)&mem, cv.off));
            int rc = st.init(next_bytes + (size_t)c.vocab + SA_MAX_PATTERN_STATES + S * 2 * sizeof(int) + 4096);
            if (!rc) rc = (int)hipMemsetAsync(mem, 0, cv.off, s);
            if (rc) { st.destroy(); (void)hipFree(mem); return rc; }
            st_pat = st;
            pat_arena = mem;
            slot_state = reinterpret_cast<int*>(mem + o_slot);
            pat_tok_class = reinterpret_cast<uint8_t*>(mem + o_cls);
            pat_state_mask = reinterpret_cast<uint8_t*>(mem + o_mask);
            pat_next_state = reinterpret_cast<uint16_t*>(mem + o_next);
        }
        st_pat.begin();
        const uint8_t* dc = st_pat.put(tok_class, (size_t)c.vocab);
        const uint8_t* dm = st_pat.put(state_mask, (size_t)n_states);
        const uint16_t* dn = st_pat.put(next_state, n_next);
        if (!dc || !dm || !dn) return SA_ERR_NOMEM;
        int rc = st_pat.flush(s);
        if (rc) return rc;
        SA_HIP(hipMemsetAsync(slot_state, 0xff, S * sizeof(int), s));
        SA_HIP(hipMemcpyAsync(pat_tok_class, dc, (size_t)c.vocab, hipMemcpyDeviceToDevice, s));
        SA_HIP(hipMemcpyAsync(pat_state_mask, dm, (size_t)n_states, hipMemcpyDeviceToDevice, s));
        SA_HIP(hipMemcpy2DAsync(pat_next_state, SA_MAX_PATTERN_CLASSES * sizeof(uint16_t), dn, n_classes * sizeof(uint16_t),
                                n_classes * sizeof(uint16_t), n_states, hipMemcpyDeviceToDevice, s));
        if (pat_states == 0) drop_graphs();                 // only once the new tables are on their way: a refused call changes nothing
        pat_states = n_states;
        pat_classes = n_classes;
        return SA_OK;
    }
    int patterns_off(hipStream_t s) {
        if (pat_states == 0) return SA_OK;
        drop_graphs();
        pat_states = pat_classes = 0;
        SA_HIP(hipMemsetAsync(slot_state, 0xff, (size_t)c.max_slots * sizeof(int), s));
        return SA_OK;
    }
    // Start states of the slots about to be prefilled (-1 = no pattern; the slot's mask id is then left alone).
    int set_slot_patterns(const int32_t* slots, const int32_t* states, int n, hipStream_t s) override {
        if (n <= 0) return n < 0 ? SA_ERR_ARG : SA_OK;
        if (n > c.max_slots) return SA_ERR_ARG;
        if (pat_states == 0) return SA_ERR_STATE;
        if (check_slots(slots, n, [&](int i) { return states[i] >= -1 && states[i] < pat_states; })) return SA_ERR_ARG;
        st_pat.begin();
        const int* ds = st_pat.put(slots, n);
        const int* dt = st_pat.put(states, n);
        if (!ds || !dt) return SA_ERR_NOMEM;
        int rc = st_pat.flush(s);
        if (rc) return rc;
        hipLaunchKernelGGL(set_slot_patterns_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, ds, dt, pat_state_mask, slot_state, slot_mask, n);
        return (int)hipGetLastError();
    }
    int copy_slot_states(int32_t* dst, hipStream_t s) override { return copy_states(dst, slot_state, s); }

    // The automaton of lexicon-guided decoding (lexicon.h), from host arrays. Everything is checked before anything is enqueued or
    // allocated: the kernels read the tables unchecked. New tables set every slot's state back to -1.
    int set_lexicon(const int32_t* edge_off, const int32_t* edge_tok, const int32_t* edge_next, const uint8_t* flags, int n_states, int n_edges,
                    int nop, hipStream_t s) override {
        if (n_states < 0 || n_states > SA_MAX_LEXICON_STATES || n_edges < 0 || n_edges > SA_MAX_LEXICON_EDGES) return SA_ERR_ARG;
        if (n_states == 0) return lexicon_off(s);
        if (!edge_off || !flags || (n_edges > 0 && (!edge_tok || !edge_next))) return SA_ERR_ARG;
        if (n_token_masks == 0 || excluded(M_LEXICON)) return SA_ERR_STATE;
        if (csr_check(edge_off, edge_tok, edge_next, n_states, n_edges, c.vocab) ||
            lexicon_check(edge_off, flags, n_states, c.vocab, c.eos_token_id, c.pad_token_id, nop))
            return SA_ERR_ARG;
        int rc;
        if (!slot_lex_state) {                              // first tables: the per-slot state and its staging, or nothing
            int* mem = nullptr;
            Stager st;
            SA_HIP(hipMalloc((void**)&mem, (size_t)c.max_slots * sizeof(int)));
            rc = st.init((size_t)c.max_slots * 2 * sizeof(int) + 4096);
            if (!rc) rc = (int)hipMemset(mem, 0xff, (size_t)c.max_slots * sizeof(int));      // every slot -1, whatever fails below
            if (rc) { st.destroy(); (void)hipFree(mem); return rc; }
            st_lex = st; slot_lex_state = mem;
        }
        if (!mask_dyn_rows && (rc = grow_mask_arena(s))) return rc;
        if ((rc = place_tables(lex, lex_states, edge_off, edge_tok, edge_next, flags, n_states, n_edges, s))) return rc;
        SA_HIP(hipMemsetAsync(slot_lex_state, 0xff, (size_t)c.max_slots * sizeof(int), s));
        if (lex_states == 0 || nop != lex_nop) drop_graphs();      // on <-> off, and the by-value no-output id of the step launch
        lex_states = n_states;
        lex_nop = nop;
        return SA_OK;
    }
    // The mask arena with max_slots dynamic rows behind the static ones: a new block of the same layout, the old contents copied in
    // stream order. Called once per handle, from the set_lexicon that switches the feature on for the first time, which drops every
    // captured step anyway; no address moves after it.
    int grow_mask_arena(hipStream_t s) {
        const size_t words = mask_words(), table_bytes = (size_t)SA_MAX_TOKEN_MASKS * words * sizeof(uint32_t),
                     dyn_bytes = (size_t)c.max_slots * words * sizeof(uint32_t);
        Carve cv;
        const size_t o_slot = cv.take((size_t)c.max_slots * sizeof(int)), o_table = cv.take(table_bytes + dyn_bytes);
        char* mem = nullptr;
        SA_HIP(hipMalloc((void**)&mem, cv.off));
        int rc = (int)hipMemcpyAsync(mem + o_slot, slot_mask, (size_t)c.max_slots * sizeof(int), hipMemcpyDeviceToDevice, s);
        if (!rc) rc = (int)hipMemcpyAsync(mem + o_table, mask_table, table_bytes, hipMemcpyDeviceToDevice, s);
        if (!rc) rc = (int)hipMemsetAsync(mem + o_table + table_bytes, 0, dyn_bytes, s);
        if (!rc) rc = (int)hipDeviceSynchronize();          // the copies are done and nothing in flight reads the old block
        if (rc) { (void)hipFree(mem); return rc; }
        drop_graphs();
        (void)hipFree(mask_arena);
        mask_arena = mem;
        slot_mask = reinterpret_cast<int*>(mem + o_slot);
        mask_table = reinterpret_cast<uint32_t*>(mem + o_table);
        mask_dyn_rows = true;
        return SA_OK;
    }
    // Room for a feature's tables, then the tables (set_lexicon, set_boost). A block that moved drops captured steps, which hold the
    // old addresses, and switches the feature off (states_on = 0) until the new tables are on their way.
    int place_tables(CsrDevice& t, int& states_on, const int32_t* edge_off, const int32_t* edge_tok, const int32_t* edge_next,
                     const uint8_t* flags, int n_states, int n_edges, hipStream_t s) {
        bool moved = false;
        const int rc = t.grow(n_states, n_edges, &moved);
        if (rc) return rc;
        if (moved) { drop_graphs(); states_on = 0; }
        return t.upload(edge_off, edge_tok, edge_next, flags, n_states, n_edges, s);
    }
    int lexicon_off(hipStream_t s) {
        if (lex_states == 0) return SA_OK;
        drop_graphs();
        lex_states = 0;
        SA_HIP(hipMemsetAsync(slot_lex_state, 0xff, (size_t)c.max_slots * sizeof(int), s));
        return SA_OK;
    }
    // Start states of the slots about to be prefilled (-1 = no lexicon; the slot's mask id and row are then left alone).
    int set_slot_lexicon(const int32_t* slots, const int32_t* states, int n, hipStream_t s) override {
        if (n <= 0) return n < 0 ? SA_ERR_ARG : SA_OK;
        if (n > c.max_slots) return SA_ERR_ARG;
        if (lex_states == 0) return SA_ERR_STATE;
        if (check_slots(slots, n, [&](int i) { return states[i] >= -1 && states[i] < lex_states; })) return SA_ERR_ARG;
        st_lex.begin();
        const int* ds = st_lex.put(slots, n);
        const int* dt = st_lex.put(states, n);
        if (!ds || !dt) return SA_ERR_NOMEM;
        int rc = st_lex.flush(s);
        if (rc) return rc;
        return launch_lexicon_start(lex_args(), ds, dt, n, s);
    }
    int copy_lexicon_states(int32_t* dst, hipStream_t s) override { return copy_states(dst, slot_lex_state, s); }

    // The automaton of boosted decoding (boost.h), from host arrays. Everything is checked before anything is enqueued or allocated: the
    // kernels read the tables unchecked. New tables set every slot back to "not boosted".
    int set_boost(const int32_t* edge_off, const int32_t* edge_tok, const int32_t* edge_next, int n_states, int n_edges, int out_state,
                  int word_row, hipStream_t s) override {
        if (n_states < 0 || n_states > SA_MAX_LEXICON_STATES || n_edges < 0 || n_edges > SA_MAX_LEXICON_EDGES) return SA_ERR_ARG;
        if (n_states == 0) return boost_off(s);
        if (!edge_off || (n_edges > 0 && (!edge_tok || !edge_next))) return SA_ERR_ARG;
        if (n_token_masks == 0 || excluded(M_BOOST)) return SA_ERR_STATE;
        if (!head2_ok() || cdiv(c.vocab, 64) > 4 * SA_HEAD_THREADS) return SA_ERR_STATE;      // the fallback head would have to run
        if (csr_check(edge_off, edge_tok, edge_next, n_states, n_edges, c.vocab) ||
            boost_check(edge_off, edge_tok, n_states, n_edges, out_state, word_row, n_token_masks, c.eos_token_id, c.pad_token_id))
            return SA_ERR_ARG;
        int rc;
        if (!bst_slots.dev) {                               // first tables: the per-slot arrays, record B's partials, the outputs -- or nothing
            const size_t S = c.max_slots, out_b = (size_t)SA_MAX_STEPS * S * 4;
            Carve cv;
            const size_t o_state = cv.take(S * 4), o_root = cv.take(S * 4), o_beta = cv.take(S * 4),
                         o_amax = cv.take(S * (size_t)cdiv(c.vocab, 32) * sizeof(float4)), o_ptok = cv.take(out_b), o_pprob = cv.take(out_b);
            DevBlock b;
            Stager st;
            std::vector<float> inf(S, INFINITY);
            rc = b.alloc(cv.off, 2 * out_b);
            if (!rc) rc = st.init(S * 3 * sizeof(int) + 4096);
            if (!rc) rc = (int)hipMemset(b.dev + o_state, 0xff, o_beta - o_state);                    // state and root -1
            if (!rc) rc = (int)hipMemcpy(b.dev + o_beta, inf.data(), S * 4, hipMemcpyHostToDevice);      // beta +inf
            if (rc) { st.destroy(); b.release(); return rc; }
            bst_slots = b; st_bst = st;
            slot_bst_state = reinterpret_cast<int*>(b.dev + o_state);
            slot_bst_root = reinterpret_cast<int*>(b.dev + o_root);
            slot_bst_beta = reinterpret_cast<float*>(b.dev + o_beta);
            amax_b = reinterpret_cast<float4*>(b.dev + o_amax);
            plain_token = reinterpret_cast<int*>(b.dev + o_ptok);
            plain_prob = reinterpret_cast<float*>(b.dev + o_pprob);
            StepOutputs& o = outs[STEPS_BOOST];
            o.add(plain_token, 4); o.add(plain_prob, 4);
            o.host = b.host;
        }
        if (!mask_dyn_rows && (rc = grow_mask_arena(s))) return rc;
        if ((rc = place_tables(bst, bst_states, edge_off, edge_tok, edge_next, nullptr, n_states, n_edges, s))) return rc;
        if ((rc = reset_boost_slots(s))) return rc;
        if (bst_states == 0 || out_state != bst_out || word_row != bst_word_row) drop_graphs();      // on <-> off, and the by-value ids of the step launch
        bst_states = n_states;
        bst_out = out_state;
        bst_word_row = word_row;
        return SA_OK;
    }
    int reset_boost_slots(hipStream_t s) {                  // every slot: state and root -1, beta +inf (0x7f800000)
        SA_HIP(hipMemsetAsync(slot_bst_state, 0xff, (size_t)c.max_slots * sizeof(int), s));
        SA_HIP(hipMemsetAsync(slot_bst_root, 0xff, (size_t)c.max_slots * sizeof(int), s));
        SA_HIP(hipMemsetD32Async((hipDeviceptr_t)slot_bst_beta, 0x7f800000, (size_t)c.max_slots, s));
        return SA_OK;
    }
    int boost_off(hipStream_t s) {
        if (bst_states == 0) return SA_OK;
        drop_graphs();
        bst_states = 0;
        return reset_boost_slots(s);
    }
    // Roots and boosts of the slots about to be prefilled (root -1 = not boosted: beta +inf, the slot's mask id and row are left alone).
    int set_slot_boost(const int32_t* slots, const int32_t* roots, const float* betas, int n, hipStream_t s) override {
        if (n <= 0) return n < 0 ? SA_ERR_ARG : SA_OK;
        if (n > c.max_slots) return SA_ERR_ARG;
        if (bst_states == 0) return SA_ERR_STATE;
        if (check_slots(slots, n, [&](int i) {              // a boosted slot's beta: finite, >= 0 (NaN fails both)
                return roots[i] >= -1 && roots[i] < bst_states && (roots[i] < 0 || (betas[i] >= 0.f && betas[i] < INFINITY));
            }))
            return SA_ERR_ARG;
        st_bst.begin();
        const int* ds = st_bst.put(slots, n);
        const int* dr = st_bst.put(roots, n);
        const float* db = st_bst.put(betas, n);
        if (!ds || !dr || !db) return SA_ERR_NOMEM;
        int rc = st_bst.flush(s);
        if (rc) return rc;
        return launch_boost_start(bst_args(), ds, dr, db, n, s);
    }
    int copy_boost_states(int32_t* dst, hipStream_t s) override { return copy_states(dst, slot_bst_state, s); }

    // Alternatives on / off. Memory on the first switch-on, or nothing (a failure leaves the handle as it was); switching drops captured
    // steps, which hold the other lm_head kernel and the head's null / non-null (max, total) pointer.
    int set_alternatives(int on) override {
        if (on != 0 && on != 1) return SA_ERR_ARG;
        if (on && excluded(M_ALTS)) return SA_ERR_STATE;
        if (on) {
            const int rc = ensure_alt_arena();
            if (rc) return rc;
        }
        if ((on != 0) != alts) drop_graphs();
        alts = on != 0;
        return SA_OK;
    }
    int ensure_alt_arena() {
        if (alt_arena.dev) return SA_OK;
        const size_t S = c.max_slots, cell = SA_MAX_ALTERNATIVES * 4, out_b = (size_t)SA_MAX_STEPS * S * cell;
        Carve cv;
        const size_t o_part = cv.take(S * (size_t)cdiv(c.vocab, 64) * SA_MAX_ALTERNATIVES * sizeof(float2)), o_bt = cv.take(S * sizeof(float2)),
                     o_tok = cv.take(out_b), o_prob = cv.take(out_b);
        const int rc = alt_arena.alloc(cv.off, 2 * out_b);
        if (rc) return rc;
        char* mem = alt_arena.dev;
        alt_part = reinterpret_cast<float2*>(mem + o_part);
        best_tot = reinterpret_cast<float2*>(mem + o_bt);
        alt_token = reinterpret_cast<int*>(mem + o_tok);
        alt_prob = reinterpret_cast<float*>(mem + o_prob);
        StepOutputs& o = outs[STEPS_ALTS];
        o.add(alt_token, cell); o.add(alt_prob, cell);
        o.host = alt_arena.host;
        return SA_OK;
    }

    // Beam search on (width 2..SA_MAX_BEAMS) / off (0). Memory on the first switch-on, or nothing (a failure leaves the handle as it was);
    // switching drops captured steps, which hold the other lm_head kernel, the fused or unfused head and no selection / fork launches.
    int set_beam(int width, int nop_id) override {
        if (width != 0 && (width < 2 || width > SA_MAX_BEAMS || width > c.max_slots)) return SA_ERR_ARG;
        if (width && excluded(M_BEAM)) return SA_ERR_STATE;
        if (width) {
            int rc = ensure_alt_arena();
            if (rc) return rc;
            if (!beam_arena.dev) {
                const size_t S = c.max_slots, out_b = (size_t)SA_MAX_STEPS * S * 4;
                Carve cv;
                size_t o_slot[6], o_out[5];
                for (size_t& v : o_slot) v = cv.take(S * 4);
                for (size_t& v : o_out) v = cv.take(out_b);
                DevBlock b;
                if ((rc = b.alloc(cv.off, 5 * out_b))) return rc;
                if ((rc = (int)hipMemset(b.dev + o_slot[3], 0xff, S * 4))) { b.release(); return rc; }      // fork_src -1: nothing to copy
                beam_arena = b;
                auto ints = [&](size_t o) { return reinterpret_cast<int*>(b.dev + o); };
                auto floats = [&](size_t o) { return reinterpret_cast<float*>(b.dev + o); };
                beam_score = floats(o_slot[0]); beam_fin = ints(o_slot[1]); beam_prompt = ints(o_slot[2]);
                fork_src = ints(o_slot[3]); fork_base = ints(o_slot[4]); fork_len = ints(o_slot[5]);
                beam_token = ints(o_out[0]); beam_parent = ints(o_out[1]); beam_rank = ints(o_out[2]);
                beam_prob = floats(o_out[3]); beam_logp = floats(o_out[4]);
                StepOutputs& o = outs[STEPS_BEAM];
                for (size_t v : o_out) o.add(b.dev + v, 4);       // token, parent, rank, probability, log-probability
                o.host = b.host;
            }
        }
        if (width != beam) drop_graphs();
        beam = width;
        beam_nop = nop_id;
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

    // Forced decoding on / off. Memory on the first switch-on, or nothing (a failure leaves the handle as it was); switching drops captured
    // steps, which hold the other lm_head kernel and the head's empty / filled ForcedHead. Switch-off sets the table back to -1.
    int set_forced(int on) override {
        if (on != 0 && on != 1) return SA_ERR_ARG;
        if (on && excluded(M_FORCED)) return SA_ERR_STATE;
        const size_t S = c.max_slots, table_bytes = S * SA_MAX_FORCED_TOKENS * sizeof(int), out_b = (size_t)SA_MAX_STEPS * S * 4;
        if (on && !forced_arena.dev) {
            Carve cv;
            const size_t o_table = cv.take(table_bytes), o_cursor = cv.take(S * sizeof(int)), o_flogit = cv.take(S * sizeof(float)),
                         o_gtok = cv.take(out_b), o_gprob = cv.take(out_b), o_logp = cv.take(out_b);
            DevBlock b;
            Stager st;
            int rc = b.alloc(cv.off, 3 * out_b);
            if (!rc) rc = st.init(table_bytes + (2 * S + 1) * sizeof(int) + 4096);
            if (!rc) rc = (int)hipMemset(b.dev + o_table, 0xff, table_bytes);           // every slot free-running
            if (rc) { st.destroy(); b.release(); return rc; }
            st_forced = st;
            forced_arena = b;
            forced_table = reinterpret_cast<int*>(b.dev + o_table);
            forced_cursor = reinterpret_cast<int*>(b.dev + o_cursor);
            flogit = reinterpret_cast<float*>(b.dev + o_flogit);
            greedy_token = reinterpret_cast<int*>(b.dev + o_gtok);
            greedy_prob = reinterpret_cast<float*>(b.dev + o_gprob);
            forced_logprob = reinterpret_cast<float*>(b.dev + o_logp);
            StepOutputs& o = outs[STEPS_FORCED];
            o.add(greedy_token, 4); o.add(greedy_prob, 4); o.add(forced_logprob, 4);
            o.host = b.host;
        }
        if (!on && forcing) {
            SA_HIP(hipDeviceSynchronize());                                 // (a switch, not a step: no line is in flight)
            SA_HIP(hipMemset(forced_table, 0xff, table_bytes));
            SA_HIP(hipDeviceSynchronize());
        }
        if ((on != 0) != forcing) drop_graphs();
        forcing = on != 0;
        return SA_OK;
    }
    // The forced ids of the slots about to be prefilled: slot slots[i] gets tokens[offsets[i] .. offsets[i + 1]), -1 behind them, cursor 0.
    int set_forced_tokens(const int32_t* slots, const int32_t* tokens, const int32_t* offsets, int n, hipStream_t s) override {
        if (n < 0 || n > c.max_slots) return SA_ERR_ARG;
        if (!forcing) return SA_ERR_STATE;
        if (n == 0) return SA_OK;
        if (offsets[0] < 0) return SA_ERR_ARG;
        if (check_slots(slots, n, [&](int i) {
                const int len = offsets[i + 1] - offsets[i];
                if (len < 0 || len > SA_MAX_FORCED_TOKENS) return false;
                for (int j = offsets[i]; j < offsets[i + 1]; ++j)
                    if (tokens[j] < 0 || tokens[j] >= c.vocab) return false;
                return true;
            }))
            return SA_ERR_ARG;
        st_forced.begin();
        const int* ds = st_forced.put(slots, n);
        const int* dof = st_forced.put(offsets, (size_t)n + 1);
        const int* dt = st_forced.put(tokens + offsets[0], (size_t)(offsets[n] - offsets[0]));
        if (!ds || !dof || !dt) return SA_ERR_NOMEM;
        int rc = st_forced.flush(s);
        if (rc) return rc;
        hipLaunchKernelGGL(set_forced_tokens_kernel, dim3(n), dim3(256), 0, s, ds, dt - offsets[0], dof, forced_table, forced_cursor,
                           SA_MAX_FORCED_TOKENS);
        return (int)hipGetLastError();
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
        if (!mx_arena.dev) {
            const size_t S = c.max_slots;
            Carve cv;
            const size_t o1 = cv.take(S * Hd), o2 = cv.take(S * Hd / 32), o3 = cv.take(S * A), o4 = cv.take(S * A / 32), o5 = cv.take(S * I),
                         o6 = cv.take(S * I / 32), o7 = cv.take(S * Hd), o8 = cv.take(S * Hd / 32);
            const int rc = mx_arena.alloc(cv.off, 0);
            if (rc) return rc;
            uint8_t* b = reinterpret_cast<uint8_t*>(mx_arena.dev);
            dh8 = b + o1; sdh = b + o2; dattn8 = b + o3; sattn = b + o4; dmlp8 = b + o5; smlp = b + o6; dlast8 = b + o7; slast = b + o8;
        }
        mxw.resize(n);
        for (int i = 0; i < n; ++i) mxw[i] = reinterpret_cast<const uint8_t*>(tbl[i]);
        drop_graphs();                                                  // captured steps hold the old launch arguments
        return SA_OK;
    }


    bool head2_ok() const { return sa::head2_ok(c.dec_hidden, mx()); }       // the rule of launch_decode_embed / launch_head (kernels.h)
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
        if (fan_offsets[0] != 0) return SA_ERR_ARG;
        for (int i = 0; i < n_seqs; ++i)
            if (fan_offsets[i + 1] <= fan_offsets[i] || fan_offsets[i + 1] > c.max_slots) return SA_ERR_ARG;      // at least the lead; max_slots in all
        if (check_slots(fan_slots, fan_offsets[n_seqs], [](int) { return true; })) return SA_ERR_ARG;
        std::vector<int32_t> leads(n_seqs);
        for (int i = 0; i < n_seqs; ++i) leads[i] = fan_slots[fan_offsets[i]];
        return prefill_fan(tiles, grid_hw, n_images, input_ids, seq_offsets, leads.data(), n_seqs, fan_offsets, fan_slots, s);
    }

    // ---------------------------------------------------------------------------------------- prompt store
    // Prompts that outlive their slots (surya_rec_prefill_keep / surya_rec_restore; kv_store.h): [K | V][layer][kv_head][store_cap][D] and
    // the hidden rows [store_cap][dec_hidden], in one lazily allocated block. store_live is the host's table of entries, first -> len.
    // Decode steps never read the store, so no captured step holds one of its addresses and growing it drops none.
    DevBlock store;
    T *store_k = nullptr, *store_v = nullptr, *store_h = nullptr;
    int store_cap = 0;
    std::map<int, int> store_live;
    static bool store_free(const std::map<int, int>& live, int first, int len) {      // [first, first + len) touches no entry of `live`
        auto it = live.lower_bound(first);
        if (it != live.end() && it->first < first + len) return false;
        if (it == live.begin()) return true;
        --it;                                               // the entry below: it must end at or before `first`
        return it->first + it->second <= first;
    }
    int reserve_prompts(int rows, hipStream_t s) override {
        if (rows < 0) return SA_ERR_ARG;
        if (rows <= store_cap) return SA_OK;
        const size_t runs = (size_t)c.dec_layers * c.dec_kv_heads, row_b = (size_t)c.dec_head_dim * sizeof(T), hid_b = (size_t)c.dec_hidden * sizeof(T);
        Carve cv;
        const size_t o_k = cv.take(runs * rows * row_b), o_v = cv.take(runs * rows * row_b), o_h = cv.take((size_t)rows * hid_b);
        DevBlock nb;
        int rc = nb.alloc(cv.off, 0);
        if (rc) return rc;
        if (store_cap > 0) {      // every run's old rows to the front of its new run, in stream order; then nothing in flight reads the old block
            const size_t old_run = (size_t)store_cap * row_b, new_run = (size_t)rows * row_b;
            rc = (int)hipMemcpy2DAsync(nb.dev + o_k, new_run, store_k, old_run, old_run, runs, hipMemcpyDeviceToDevice, s);
            if (!rc) rc = (int)hipMemcpy2DAsync(nb.dev + o_v, new_run, store_v, old_run, old_run, runs, hipMemcpyDeviceToDevice, s);
            if (!rc) rc = (int)hipMemcpyAsync(nb.dev + o_h, store_h, (size_t)store_cap * hid_b, hipMemcpyDeviceToDevice, s);
        }
        if (!rc) rc = (int)hipDeviceSynchronize();
        if (rc) { nb.release(); return rc; }
        store.release();
        store = nb;
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
        for (int i = 0; i < n_seqs; ++i) {
            const int f = keep_first[i], L = seq_offsets[i + 1] - seq_offsets[i];
            if (f == -1) continue;
            if (f < 0 || L <= 0 || L > store_cap || f > store_cap - L || !store_free(live, f, L)) return SA_ERR_ARG;
            live[f] = L;
        }
        if (live.size() == store_live.size()) keep_first = nullptr;      // nothing named: surya_rec_prefill
        const int rc = prefill_fan(tiles, grid_hw, n_images, input_ids, seq_offsets, slot_ids, n_seqs, nullptr, nullptr, s, keep_first);
        if (!rc) store_live.swap(live);
        return rc;
    }
    // surya_rec_restore: everything about the entries and the fans is checked here, before anything is enqueued or changed.
    int restore(const int32_t* first, const int32_t* fan_offsets, const int32_t* fan_slots, int n, hipStream_t s) override {
        if (n <= 0) return SA_OK;
        if (n > c.max_slots) return SA_ERR_ARG;
        if (kv8) return SA_ERR_STATE;
        if (fan_offsets[0] != 0) return SA_ERR_ARG;
        for (int i = 0; i < n; ++i) {
            if (fan_offsets[i + 1] <= fan_offsets[i] || fan_offsets[i + 1] > c.max_slots) return SA_ERR_ARG;
            if (beam > 0 && fan_offsets[i + 1] - fan_offsets[i] != 1) return SA_ERR_ARG;           // beam search owns whole groups and forks on its own
            if (!store_live.count(first[i])) return SA_ERR_ARG;
        }
        const int F = fan_offsets[n];
        if (check_slots(fan_slots, F, [&](int j) { return beam == 0 || (fan_slots[j] % beam == 0 && fan_slots[j] + beam <= c.max_slots); }))
            return SA_ERR_ARG;
        if (h_len.size() < (size_t)c.max_slots) h_len.resize(c.max_slots, 0);
        std::vector<int> lens(n), f_lens, f_first;
        for (int i = 0; i < n; ++i) {
            lens[i] = store_live[first[i]];
            for (int j = fan_offsets[i]; j < fan_offsets[i + 1]; ++j) {
                for (int b = 0; b < std::max(beam, 1); ++b) h_len[fan_slots[j] + b] = lens[i];
                f_lens.push_back(lens[i]); f_first.push_back(first[i]);
            }
        }
        int rc;
        st.begin();
        const int* d_first = st.put(first, n);
        const int* d_lens = st.put(lens);
        const int* d_foff = st.put(fan_offsets, n + 1);
        const int* d_fslots = st.put(fan_slots, F);
        const int* d_flens = st.put(f_lens);
        const int* d_ffirst = st.put(f_first);
        if (!d_first || !d_lens || !d_foff || !d_fslots || !d_flens || !d_ffirst) return SA_ERR_NOMEM;
        if ((rc = st.flush(s))) return rc;
        hipLaunchKernelGGL(set_slot_state_kernel, dim3(cdiv(F, 256)), dim3(256), 0, s, d_fslots, d_flens, kv_len, F);
        if ((rc = launch_kv_restore<T>(kcache, vcache, store_k, store_v, d_first, d_lens, d_foff, d_fslots, n, F, c.dec_layers, c.max_slots,
                                       c.dec_kv_heads, c.max_kv_len, c.dec_head_dim, store_cap, s))) return rc;
        if ((rc = heads(F, d_ffirst, d_fslots, 0, 0, false, s, false, store_h)) || beam == 0) return rc;
        return beam_step(d_fslots, 1, n, 0, 1, s);          // the B best first tokens, and the prompt's rows to the group's other slots
    }
    int drop_prompts(const int32_t* first, int n) override {
        std::set<int> named;
        for (int i = 0; i < n; ++i)
            if (!store_live.count(first[i]) || !named.insert(first[i]).second) return SA_ERR_ARG;
        for (int f : named) store_live.erase(f);
        return SA_OK;
    }
    int prompt_store_info(int32_t* cap_rows, int32_t* live_entries) override {
        *cap_rows = store_cap; *live_entries = (int32_t)store_live.size();
        return SA_OK;
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

    int set_active(const int32_t* slots, int n, hipStream_t s) override {
        if (n < 0 || n > c.max_slots) return SA_ERR_ARG;
        n_active = n;
        for (int i = 0; i < n; ++i)
            if (slots[i] < 0 || slots[i] >= c.max_slots) return SA_ERR_ARG;
        if (beam > 0) {                                     // whole groups, ascending
            if (n % beam) return SA_ERR_ARG;
            for (int i = 0; i < n; ++i) {
                const int lead = slots[i - i % beam];
                if (lead % beam || slots[i] != lead + i % beam || (i >= beam && i % beam == 0 && lead <= slots[i - beam])) return SA_ERR_ARG;
            }
        }
        h_active.assign(slots, slots + n);
        if (n == 0) return SA_OK;
        st_small.begin();
        const int* d = st_small.put(slots, n);
        if (!d) return SA_ERR_NOMEM;
        int rc = st_small.flush(s);
        if (rc) return rc;
        SA_HIP(hipMemcpyAsync(active_dev, d, n * sizeof(int), hipMemcpyDeviceToDevice, s));
        return SA_OK;
    }

    bool can_fuse_embed() const {       // greedy_head2_kernel's fused tail: two 4-element chunks per thread, lm_head partials in registers
        return tuning().fuse_embed && head2_ok() && c.dec_hidden <= 2 * 4 * SA_HEAD_THREADS && cdiv(c.vocab, 320) <= 4 * SA_HEAD_THREADS &&
               cdiv(c.vocab, 64) <= 4 * SA_HEAD_THREADS;
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
        int rc = decode_steps(n_steps, StepOutputs::ring_step(ring), s);
        if (rc) return rc;
        for (int k = 0; k < STEPS_SETS; ++k) {
            outs[k].mirrored[ring] = false;                 // a set that is off mirrors nothing: wait_steps refuses this ring half
            if (steps_on((StepSet)k) && (rc = outs[k].mirror(ring, n_steps, s))) return rc;
        }
        SA_HIP(hipEventRecord(ev_ring[ring], s));
        return SA_OK;
    }

    // The fields of one set for the steps read_outputs / wait_outputs return, same [step][slot] indexing. A set that is off is refused,
    // and so is a ring half whose decode_async was enqueued while the set was off.
    int wait_steps(StepSet set, int n_steps, int ring, std::initializer_list<void*> dst) override {
        if (n_steps < 0 || n_steps > SA_MAX_STEPS / 2 || ring < 0 || ring > 1) return SA_ERR_ARG;
        if (!steps_on(set) || !outs[set].mirrored[ring]) return SA_ERR_STATE;
        SA_HIP(hipEventSynchronize(ev_ring[ring]));
        outs[set].wait(ring, n_steps, dst.begin());
        return SA_OK;
    }
    int read_steps(StepSet set, int n_steps, std::initializer_list<void*> dst, hipStream_t s) override {
        if (n_steps <= 0 || n_steps > SA_MAX_STEPS) return SA_ERR_ARG;
        if (!steps_on(set)) return SA_ERR_STATE;
        return outs[set].read(n_steps, dst.begin(), s);
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

    int set_next_tokens(const int32_t* slots, const int32_t* toks, int n, hipStream_t s) override {
        if (n <= 0) return SA_OK;
        st_small.begin();
        const int* ds = st_small.put(slots, n);
        const int* dt = st_small.put(toks, n);
        if (!dt) return SA_ERR_NOMEM;
        int rc = st_small.flush(s);
        if (rc) return rc;
        hipLaunchKernelGGL(set_next_tokens_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, ds, dt, next_token, n);
        return (int)hipGetLastError();
    }
};

}  // namespace sa
