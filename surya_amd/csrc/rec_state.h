// RecBase: the half of the recognition engine that does not depend on the compute dtype -- staging, device blocks, step-output sets,
// the host checks, every decoding mode's state and setters, the graph cache, the prompt store's table. RecModel<T> (rec_engine.h) derives
// from it and holds only what names T. The rule: a member moves here iff its body names neither T nor a function or kernel templated on
// T ("Engine state"). Compiled once per translation unit that includes it, not once per dtype.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <map>
#include <set>
#include <vector>

#include "../../include/surya_amd.h"
#include "gemm.h"
#include "gemm_mx.h"
#include "kernels.h"
#include "decode_attn_kv8.h"
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
        *this = Stager();
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

// The one owner of memory the engine allocates: a device block, (host_bytes > 0) a pinned host block and (stage_bytes > 0) a Stager --
// all of them, or nothing. The device block is zeroed unless zero == false, then `fills` sets 32-bit words (0xffffffff: ints of -1 /
// every mask bit; 0x7f800000: +inf), and the device is idle when alloc returns: whatever stream uses the block next finds it filled.
// A failure leaves *this as it was. Addresses never move: a larger block is a new DevBlock swapped in by the caller (CsrDevice::grow).
struct DevBlock {
    struct Fill { size_t off, bytes; uint32_t word; };
    char* dev = nullptr;
    char* host = nullptr;
    Stager st;
    int alloc(size_t dev_bytes, size_t host_bytes = 0, size_t stage_bytes = 0, std::initializer_list<Fill> fills = {}, bool zero = true) {
        DevBlock nb;
        int rc = (int)hipMalloc((void**)&nb.dev, dev_bytes);
        if (!rc && host_bytes) rc = (int)hipHostMalloc((void**)&nb.host, host_bytes, hipHostMallocDefault);
        if (!rc && stage_bytes) rc = nb.st.init(stage_bytes);
        if (!rc && zero) rc = (int)hipMemset(nb.dev, 0, dev_bytes);
        for (const Fill& f : fills)
            if (!rc) rc = (int)hipMemsetD32((hipDeviceptr_t)(nb.dev + f.off), (int)f.word, f.bytes / 4);
        if (!rc) rc = (int)hipDeviceSynchronize();
        if (rc) { nb.release(); return rc; }             // the one "or nothing" path
        *this = nb;
        return SA_OK;
    }
    void release() {
        if (host) (void)hipHostFree(host);
        if (dev) (void)hipFree(dev);
        st.destroy();
        dev = host = nullptr;
    }
};

// A sparse automaton's tables (CSR: edge_off / edge_tok / edge_next, and a flag byte per state) in engine-owned memory sized by need,
// with their pinned staging copy: what lexicon-guided and boosted decoding each keep one of ("Sparse automata"). `arena` is
// one of the engine's blocks: the engine frees it with the others.
struct CsrDevice {
    DevBlock* arena;                                     // device tables and the staging copy, same layout, [cap_states] / [cap_edges]
    int *edge_off = nullptr, *edge_tok = nullptr, *edge_next = nullptr;      // into arena->dev
    uint8_t* flags = nullptr;
    int cap_states = 0, cap_edges = 0;
    hipEvent_t ev = nullptr;                             // the staging copy is on the device
    bool pending = false;
    explicit CsrDevice(DevBlock* b) : arena(b) {}
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
        if (rc) { nb.release(); return rc; }
        arena->release();
        *arena = nb;
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
            char* h = arena->host + (static_cast<char*>(dev) - arena->dev);
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

// ------------------------------------------------------------------------------------------- small setters
static __global__ void set_slot_state_kernel(const int* slots, const int* lens, int* kv_len, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) kv_len[slots[i]] = lens[i];
}
static __global__ void set_next_tokens_kernel(const int* slots, const int* toks, int* next_token, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) next_token[slots[i]] = toks[i];
}

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

// The step-output sets of an engine, in the order decode_async mirrors them; the fields of each in the order of its surya_rec_read_* /
// surya_rec_wait_* arguments (RecModel::init names them).
enum StepSet { STEPS_BASE = 0, STEPS_ALTS, STEPS_BEAM, STEPS_FORCED, STEPS_BOOST, STEPS_SETS };
enum Mode { M_MASKS, M_ALTS, M_FORCED, M_BEAM, M_KV8, M_MX, M_PATTERNS, M_LEXICON, M_BOOST, MODES };

// --------------------------------------------------------------------------------------------- host checks
// Plain functions without a HIP call: tools/hostcheck runs them under the host sanitizers.
// The modes that cannot be on together, and why: mode m may not be switched on while on[] holds one of its partners.
static bool modes_excluded(int m, const bool on[MODES]) {
    static constexpr int pairs[14][2] = {{M_FORCED, M_MASKS},      // forced decoding runs the unmasked partial
                                        {M_FORCED, M_ALTS},       // ... which collects no candidates
                                        {M_FORCED, M_BEAM},
                                        {M_BEAM, M_KV8},          // the KV fork copies the bf16 / fp16 / fp32 caches only
                                        {M_BEAM, M_MX},           // (beam search on the fp8 decode paths is out of scope: DESIGN.md 4l)
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
        if ((p[0] == m && on[p[1]]) || (p[1] == m && on[p[0]])) return true;
    return false;
}

// A slot list: n entries, every slot in [0, max_slots) and named once (which value would win is a race in the scatter), and also(i), the
// caller's own check of entry i, holds. SA_OK or SA_ERR_ARG.
template <typename F>
static int check_slots(const int32_t* slots, int n, int max_slots, F&& also) {
    std::vector<char> seen(max_slots, 0);
    for (int i = 0; i < n; ++i) {
        if (slots[i] < 0 || slots[i] >= max_slots || seen[slots[i]] || !also(i)) return SA_ERR_ARG;
        seen[slots[i]] = 1;
    }
    return SA_OK;
}

// The fans of surya_rec_prefill_shared / surya_rec_restore: fan i is fan_slots[fan_offsets[i] .. fan_offsets[i + 1]), the offsets start
// at 0, every fan has at least its lead, there are at most max_slots slots in all, they form a slot list, and also(i, j) holds for entry
// j of fan i. SA_OK or SA_ERR_ARG.
template <typename F>
static int check_fans(const int32_t* fan_offsets, const int32_t* fan_slots, int n, int max_slots, F&& also) {
    if (fan_offsets[0] != 0) return SA_ERR_ARG;
    for (int i = 0; i < n; ++i)
        if (fan_offsets[i + 1] <= fan_offsets[i] || fan_offsets[i + 1] > max_slots) return SA_ERR_ARG;
    int fan = 0;
    return check_slots(fan_slots, fan_offsets[n], max_slots, [&](int j) {
        while (j >= fan_offsets[fan + 1]) ++fan;
        return also(fan, j);
    });
}

// The prompt store's table is first row -> length. [first, first + len) touches no entry of `live`:
static bool store_free(const std::map<int, int>& live, int first, int len) {
    auto it = live.lower_bound(first);
    if (it != live.end() && it->first < first + len) return false;
    if (it == live.begin()) return true;
    --it;                                               // the entry below: it must end at or before `first`
    return it->first + it->second <= first;
}

// surya_rec_prefill_keep: sequence i (seq_offsets[i + 1] - seq_offsets[i] rows) goes to rows keep_first[i] .. of a store of store_cap rows,
// -1 = not kept. Every range lies inside the store and touches neither an entry of `live` nor another range; `live` gains them.
// SA_OK, or SA_ERR_ARG with `live` in an unspecified state.
static int check_keep(std::map<int, int>& live, const int32_t* keep_first, const int32_t* seq_offsets, int n_seqs, int store_cap) {
    for (int i = 0; i < n_seqs; ++i) {
        const int f = keep_first[i], L = seq_offsets[i + 1] - seq_offsets[i];
        if (f == -1) continue;
        if (f < 0 || L <= 0 || L > store_cap || f > store_cap - L || !store_free(live, f, L)) return SA_ERR_ARG;
        live[f] = L;
    }
    return SA_OK;
}

// --------------------------------------------------------------------------------------------------- state
struct RecBase {
    RecBase() = default;
    RecBase(const RecBase&) = delete;                     // lex and bst point into blk[]
    // The virtual surface is what the C entries dispatch by dtype: every body names T (the caches, the workspaces, a launch_*<T>).
    virtual ~RecBase() {
        for (DevBlock& b : blk) b.release();              // every block the engine ever allocated
        for (Stager* t : {&st, &st_small, &st_enc}) t->destroy();
        for (auto& kv : graphs) (void)hipGraphExecDestroy(kv.second);
        for (hipStream_t t : {gstream, estream}) if (t) (void)hipStreamDestroy(t);
        for (hipEvent_t e : {gev_in, gev_out, ev_ring[0], ev_ring[1], ev_ahead_in, ev_ahead_done, ev_ahead_free, lex.ev, bst.ev})
            if (e) (void)hipEventDestroy(e);
    }
    virtual int prefill(const float*, const int32_t*, int, const int32_t*, const int32_t*, const int32_t*, int, hipStream_t) = 0;
    virtual int prefill_shared(const float*, const int32_t*, int, const int32_t*, const int32_t*, const int32_t*, const int32_t*, int, hipStream_t) = 0;
    virtual int prefill_keep(const float*, const int32_t*, int, const int32_t*, const int32_t*, const int32_t*, int, const int32_t*, hipStream_t) = 0;
    virtual int restore(const int32_t*, const int32_t*, const int32_t*, int, hipStream_t) = 0;
    virtual int reserve_prompts(int, hipStream_t) = 0;
    virtual int encode_ahead(const float*, const int32_t*, int, hipStream_t) = 0;
    virtual int encode_only(const float*, const int32_t*, int, void*, hipStream_t) = 0;
    virtual int decode(int, hipStream_t) = 0;
    virtual int decode_async(int, int, hipStream_t) = 0;
    virtual int copy_last_logits(float*, int, int*, hipStream_t) = 0;
    virtual int copy_kv_rows(int, int, void*, void*, hipStream_t) = 0;
    virtual int set_mx_weights(const void* const*, int) = 0;
    virtual int set_kv_fp8(int) = 0;

    surya_rec_config c;
    std::vector<const void*> w;
    // Every device and pinned allocation of the engine is one of these blocks (DevBlock); B_MAIN comes with init, the others on the
    // first use of their mode. The destructor above frees them in one loop.
    enum Block { B_MAIN, B_MX, B_KV8, B_MASK, B_ALT, B_FORCED, B_BEAM, B_PAT, B_LEX_SLOTS, B_LEX, B_BST_SLOTS, B_BST, B_STORE, BLOCKS };
    DevBlock blk[BLOCKS];
    size_t arena_bytes = 0;
    Stager st, st_small, st_enc;                         // st_enc: plans of the look-ahead encoder (its own stream)
    hipStream_t estream = nullptr;                       // low-priority stream of the look-ahead encoder
    hipEvent_t ev_ahead_in = nullptr, ev_ahead_done = nullptr, ev_ahead_free = nullptr;
    long ahead_tokens = 0, ahead_consumed = 0;
    bool ahead_free_recorded = false;
    int *kv_len, *next_token, *active_dev, *row_len;     // [max_slots], carved by RecModel::layout
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
    // activation buffers, written by the kernels that produce the bf16 ones. Only the bf16 engine ever fills mxw.
    std::vector<const uint8_t*> mxw;
    uint8_t *dh8 = nullptr, *sdh = nullptr, *dattn8 = nullptr, *sattn = nullptr, *dmlp8 = nullptr, *smlp = nullptr, *dlast8 = nullptr,
            *slast = nullptr;
    bool mx() const { return !mxw.empty(); }
    const uint8_t* MXW(int l, int k) const { return mxw[(size_t)l * SA_MX_COUNT + k]; }
    const uint8_t* MXG(int k) const { return mxw[(size_t)c.dec_layers * SA_MX_COUNT + k]; }
    // FP8 KV cache of the decode steps (surya_rec_set_kv_fp8; decode_attn_kv8.h). Prefill keeps writing (and attending over) the
    // bf16 cache and quantises the prompt rows into these arrays; the decode steps read and append only here.
    uint8_t *k8c = nullptr, *v8tc = nullptr;     // [layer][slot][kvh][Tmax][D], [layer][slot][kvh][D][Tmax8]
    float *ksc8 = nullptr, *vsc8 = nullptr;      // [layer][slot][kvh][Tmax8]
    bool kv8 = false;
    int tmax8() const { return kv8_tmax(c.max_kv_len); }
    // Allowed-character sets (surya_rec_set_token_masks / surya_rec_set_slot_masks; TokenMask in gemm.h): a table of SA_MAX_TOKEN_MASKS
    // bit rows over the vocabulary and one row id per slot, at addresses that never change once allocated -- captured decode steps hold
    // the pointers, the contents follow the calls in stream order. n_token_masks == 0: the unmasked lm_head kernels, as ever.
    uint32_t* mask_table = nullptr;                      // [SA_MAX_TOKEN_MASKS][mask_words()]
    int* slot_mask = nullptr;                            // [max_slots], -1 = unconstrained
    int n_token_masks = 0;
    int mask_words() const { return cdiv(c.vocab, 32); }
    TokenMask token_mask(const int* d_row_slot) const { return TokenMask{mask_table, slot_mask, d_row_slot, mask_words()}; }
    // Alternatives (surya_rec_set_alternatives): per-tile candidates of the lm_head's *_TOPK epilogue, the head's (max, total) per slot and
    // the [SA_MAX_STEPS][max_slots][SA_MAX_ALTERNATIVES] outputs with their pinned mirror, allocated on the first switch-on at addresses
    // that never change afterwards. alts == false: the lm_head and head launches are the ones of a handle without this entry.
    float2* alt_part = nullptr;                          // [max_slots][cdiv(vocab, 64)][4]: 64 columns is the narrowest lm_head tile
    float2* best_tot = nullptr;                          // [max_slots]
    int* alt_token = nullptr; float* alt_prob = nullptr; // [SA_MAX_STEPS][max_slots][4]
    bool alts = false;
    // Forced decoding (surya_rec_set_forced): the id table [max_slots][SA_MAX_FORCED_TOKENS] (-1 = free-running), a cursor per slot, the
    // forced logit per lm_head row, the [SA_MAX_STEPS][max_slots] outputs and their pinned mirror, allocated on the first switch-on at
    // addresses that never change afterwards. forcing == false: the lm_head and head launches are the ones of a handle without this entry.
    int* forced_table = nullptr; int* forced_cursor = nullptr; float* flogit = nullptr;
    int* greedy_token = nullptr; float* greedy_prob = nullptr; float* forced_logprob = nullptr;   // [SA_MAX_STEPS][max_slots]
    bool forcing = false;
    ForcedCols forced_cols(const int* d_row_slot) const { return ForcedCols{forced_table, forced_cursor, d_row_slot, SA_MAX_FORCED_TOKENS, flogit}; }
    // Beam search (surya_rec_set_beam; beam.h, beam_core.h): per slot the beam's cumulative score, finished flag, its group's prompt length
    // and the fork plan of the step (source slot, first row, row count); the five [SA_MAX_STEPS][max_slots] outputs and their pinned mirror,
    // allocated on the first switch-on at addresses that never change afterwards. beam == 0: every launch is the one of a handle without
    // this entry. beam > 0: the lm_head runs its *_TOPK epilogue whatever `alts` says, and the head never fuses the next step's embedding.
    float* beam_score = nullptr; int *beam_fin = nullptr, *beam_prompt = nullptr, *fork_src = nullptr, *fork_base = nullptr, *fork_len = nullptr;   // [max_slots]
    int *beam_token = nullptr, *beam_parent = nullptr, *beam_rank = nullptr; float *beam_prob = nullptr, *beam_logp = nullptr;
    int beam = 0, beam_nop = -1;
    // Pattern-guided decoding (surya_rec_set_patterns; PatternHead in kernels.h): the automaton's three tables at their largest size and a
    // state per slot, allocated on the first call at addresses that never change afterwards -- captured decode steps hold the pointers,
    // the contents follow the calls in stream order. pat_states == 0: the head launches are the ones of a handle without this entry.
    uint8_t* pat_tok_class = nullptr;                    // [vocab]
    uint16_t* pat_next_state = nullptr;                  // [SA_MAX_PATTERN_STATES][SA_MAX_PATTERN_CLASSES]: rows always SA_MAX_PATTERN_CLASSES
                                                         // apart, so a captured head launch holds for tables of any class count
    uint8_t* pat_state_mask = nullptr;                   // [SA_MAX_PATTERN_STATES]
    int* slot_state = nullptr;                           // [max_slots], -1 = no pattern
    int pat_states = 0, pat_classes = 0;
    // Lexicon-guided decoding (surya_rec_set_lexicon; lexicon.h): the tables and a state per slot, allocated on the first call at an
    // address that never changes. Switching on or off drops captured steps. Slot s owns row SA_MAX_TOKEN_MASKS + s of the mask table; those
    // max_slots rows exist only on a handle that has seen a lexicon (mask_dyn_rows: the first set_lexicon moves the mask arena into a
    // larger block, at the one moment at which every captured step is dropped anyway; from then on its addresses never move again).
    // lex_states == 0: the handle launches exactly what a handle without this entry launches.
    CsrDevice lex{&blk[B_LEX]};
    int* slot_lex_state = nullptr;                       // [max_slots], -1 = no lexicon (B_LEX_SLOTS, whose stager takes set_slot_lexicon's lists)
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
    CsrDevice bst{&blk[B_BST]};                          // (state_flags: the zeros of the allocation, never uploaded)
    int *slot_bst_state = nullptr, *slot_bst_root = nullptr; float* slot_bst_beta = nullptr;     // [max_slots]: -1, -1, +inf = not boosted
    float4* amax_b = nullptr;                            // as RecModel::amax
    int* plain_token = nullptr; float* plain_prob = nullptr;     // [SA_MAX_STEPS][max_slots]
    int bst_states = 0, bst_out = 0, bst_word_row = 0;
    BoostArgs bst_args() const {
        return BoostArgs{TotalOps{slot_bst_root, slot_bst_beta, bst_out, bst_word_row}, csr_args(bst, slot_bst_state, -1)};
    }
    // Prompts that outlive their slots (surya_rec_prefill_keep / surya_rec_restore; kv_store.h): store_live is the host's table of the
    // entries of B_STORE, first row -> length; RecModel<T> knows the block's layout.
    int store_cap = 0;
    std::map<int, int> store_live;

    int copy_states(int32_t* dst, const int* states, hipStream_t s) const {      // the three copy_*_states
        if (!states) return SA_ERR_STATE;
        SA_HIP(hipMemcpyAsync(dst, states, (size_t)c.max_slots * sizeof(int), hipMemcpyDeviceToDevice, s));
        return SA_OK;
    }
    int copy_slot_states(int32_t* dst, hipStream_t s) { return copy_states(dst, slot_state, s); }
    int copy_lexicon_states(int32_t* dst, hipStream_t s) { return copy_states(dst, slot_lex_state, s); }
    int copy_boost_states(int32_t* dst, hipStream_t s) { return copy_states(dst, slot_bst_state, s); }
    bool topk() const { return alts || beam > 0; }       // the lm_head collects candidates and topk_combine_kernel runs
    // Which step-output sets the kernels write right now: decode_async mirrors these, read_steps / wait_steps refuse the others.
    bool steps_on(StepSet k) const { return k == STEPS_BASE || (k == STEPS_ALTS && topk()) || (k == STEPS_BEAM && beam > 0) || (k == STEPS_FORCED && forcing) || (k == STEPS_BOOST && bst_states > 0); }
    // Every setter asks excluded() before it switches its own mode on (modes_excluded above).
    bool excluded(int m) const {
        const bool on[MODES] = {n_token_masks > 0, alts, forcing, beam > 0, kv8, mx(), pat_states > 0, lex_states > 0, bst_states > 0};
        return modes_excluded(m, on);
    }
    bool head2_ok() const { return sa::head2_ok(c.dec_hidden, mx()); }       // the rule of launch_decode_embed / launch_head (kernels.h)
    bool can_fuse_embed() const {       // greedy_head2_kernel's fused tail: two 4-element chunks per thread, lm_head partials in registers
        return tuning().fuse_embed && head2_ok() && c.dec_hidden <= 2 * 4 * SA_HEAD_THREADS && cdiv(c.vocab, 320) <= 4 * SA_HEAD_THREADS &&
               cdiv(c.vocab, 64) <= 4 * SA_HEAD_THREADS;
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

    // Captured decode steps hold launch arguments AND kernel choices: any mode change (fp8 KV cache, MXFP8 weights, a tuning knob)
    // must drop them, or a replay would run the other attention kernel on a cache the new shapes no longer append to.
    void drop_graphs() {
        for (auto& kv : graphs) (void)hipGraphExecDestroy(kv.second);
        graphs.clear(); seen_keys.clear();
    }

    // What the set_slot_* calls share: n == 0 is a no-op (*ds stays null), 1 <= n <= max_slots, the mode is on, the slots form a slot
    // list whose entries pass also(i), and the slots and the call's 4-byte columns go through the block's stager on s. *ds and dcol[k]
    // are the device copies; each setter then runs its own launch.
    template <typename F>
    int stage_slot_call(Block b, bool on, const int32_t* slots, std::initializer_list<const void*> cols, int n, hipStream_t s, F&& also,
                        const int** ds, const int** dcol) {
        *ds = nullptr;
        if (n <= 0) return n < 0 ? SA_ERR_ARG : SA_OK;
        if (n > c.max_slots) return SA_ERR_ARG;
        if (!on) return SA_ERR_STATE;
        if (check_slots(slots, n, c.max_slots, also)) return SA_ERR_ARG;
        Stager& t = blk[b].st;
        t.begin();
        const int* d = t.put(slots, n);
        for (const void* col : cols)
            if (!(*dcol++ = t.put(static_cast<const int*>(col), n))) return SA_ERR_NOMEM;
        if (!d) return SA_ERR_NOMEM;
        const int rc = t.flush(s);
        if (!rc) *ds = d;
        return rc;
    }

    // The mask table of the lm_head's greedy epilogues. Every row needs an allowed id inside the vocabulary: a row without one would
    // make the head emit the "no column" index 0x7fffffff and the next step embed it. Replacing the table sets every slot back to -1 (the
    // ids named rows of the old table). Switching between the masked and the unmasked kernels drops captured steps, as set_kv_fp8 does.
    int set_token_masks(const uint32_t* masks, int n, hipStream_t s) {
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
        DevBlock& b = blk[B_MASK];
        if (!b.dev) {                                       // first table: every slot -1, every column allowed
            Carve cv;
            const size_t o_slot = cv.take((size_t)c.max_slots * sizeof(int)), o_table = cv.take(table_bytes);   // (grow_mask_arena: same layout)
            const int rc = b.alloc(cv.off, 0, table_bytes + (size_t)c.max_slots * 2 * sizeof(int) + 4096, {{0, cv.off, 0xffffffffu}}, false);
            if (rc) return rc;
            slot_mask = reinterpret_cast<int*>(b.dev + o_slot);
            mask_table = reinterpret_cast<uint32_t*>(b.dev + o_table);
        }
        b.st.begin();
        const uint32_t* d = b.st.put(masks, (size_t)n * words);
        if (!d) return SA_ERR_NOMEM;
        int rc = b.st.flush(s);
        if (rc) return rc;
        SA_HIP(hipMemsetAsync(slot_mask, 0xff, (size_t)c.max_slots * sizeof(int), s));
        SA_HIP(hipMemcpyAsync(mask_table, d, (size_t)n * words * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
        if (n_token_masks == 0) drop_graphs();              // only once the new table is on its way: a refused call changes nothing
        n_token_masks = n;
        return automata_off(s);                             // the state -> row map named rows of the old table; every slot's id is -1 again
    }
    // Mask ids of the slots about to be prefilled (-1 = unconstrained); a slot keeps its id until it is set again.
    int set_slot_masks(const int32_t* slots, const int32_t* ids, int n, hipStream_t s) {
        const int *ds, *di;
        int rc = stage_slot_call(B_MASK, n_token_masks > 0, slots, {ids}, n, s, [&](int i) { return ids[i] >= -1 && ids[i] < n_token_masks; }, &ds, &di);
        if (rc || !ds) return rc;
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
                     hipStream_t s) {
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
        DevBlock& b = blk[B_PAT];
        if (!b.dev) {                                       // first tables
            Carve cv;
            const size_t o_slot = cv.take(S * sizeof(int)), o_cls = cv.take(c.vocab), o_mask = cv.take(SA_MAX_PATTERN_STATES),
                         o_next = cv.take(next_bytes);
            const int rc = b.alloc(cv.off, 0, next_bytes + (size_t)c.vocab + SA_MAX_PATTERN_STATES + S * 2 * sizeof(int) + 4096);
            if (rc) return rc;
            slot_state = reinterpret_cast<int*>(b.dev + o_slot);
            pat_tok_class = reinterpret_cast<uint8_t*>(b.dev + o_cls);
            pat_state_mask = reinterpret_cast<uint8_t*>(b.dev + o_mask);
            pat_next_state = reinterpret_cast<uint16_t*>(b.dev + o_next);
        }
        b.st.begin();
        const uint8_t* dc = b.st.put(tok_class, (size_t)c.vocab);
        const uint8_t* dm = b.st.put(state_mask, (size_t)n_states);
        const uint16_t* dn = b.st.put(next_state, n_next);
        if (!dc || !dm || !dn) return SA_ERR_NOMEM;
        int rc = b.st.flush(s);
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
    int set_slot_patterns(const int32_t* slots, const int32_t* states, int n, hipStream_t s) {
        const int *ds, *dt;
        const int rc = stage_slot_call(B_PAT, pat_states > 0, slots, {states}, n, s, [&](int i) { return states[i] >= -1 && states[i] < pat_states; }, &ds, &dt);
        if (rc || !ds) return rc;
        hipLaunchKernelGGL(set_slot_patterns_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, ds, dt, pat_state_mask, slot_state, slot_mask, n);
        return (int)hipGetLastError();
    }

    // The automaton of lexicon-guided decoding (lexicon.h), from host arrays. Everything is checked before anything is enqueued or
    // allocated: the kernels read the tables unchecked. New tables set every slot's state back to -1.
    int set_lexicon(const int32_t* edge_off, const int32_t* edge_tok, const int32_t* edge_next, const uint8_t* flags, int n_states, int n_edges,
                    int nop, hipStream_t s) {
        if (n_states < 0 || n_states > SA_MAX_LEXICON_STATES || n_edges < 0 || n_edges > SA_MAX_LEXICON_EDGES) return SA_ERR_ARG;
        if (n_states == 0) return lexicon_off(s);
        if (!edge_off || !flags || (n_edges > 0 && (!edge_tok || !edge_next))) return SA_ERR_ARG;
        if (n_token_masks == 0 || excluded(M_LEXICON)) return SA_ERR_STATE;
        if (csr_check(edge_off, edge_tok, edge_next, n_states, n_edges, c.vocab) ||
            lexicon_check(edge_off, flags, n_states, c.vocab, c.eos_token_id, c.pad_token_id, nop))
            return SA_ERR_ARG;
        int rc;
        if (!slot_lex_state) {                              // first tables: the per-slot state, every slot -1 whatever fails below
            const size_t bytes = (size_t)c.max_slots * sizeof(int);
            if ((rc = blk[B_LEX_SLOTS].alloc(bytes, 0, 2 * bytes + 4096, {{0, bytes, 0xffffffffu}}, false))) return rc;
            slot_lex_state = reinterpret_cast<int*>(blk[B_LEX_SLOTS].dev);
        }
        if (!mask_dyn_rows && (rc = grow_mask_arena(s))) return rc;
        if ((rc = place_tables(lex, lex_states, edge_off, edge_tok, edge_next, flags, n_states, n_edges, s))) return rc;
        SA_HIP(hipMemsetAsync(slot_lex_state, 0xff, (size_t)c.max_slots * sizeof(int), s));
        if (lex_states == 0 || nop != lex_nop) drop_graphs();      // on <-> off, and the by-value no-output id of the step launch
        lex_states = n_states;
        lex_nop = nop;
        return SA_OK;
    }
    // The mask arena with max_slots dynamic (zeroed) rows behind the static ones: a new block of the same layout swapped in, the old
    // contents copied in stream order, the stager kept. Called once per handle, from the set_lexicon / set_boost that switches the feature
    // on for the first time, which drops every captured step anyway; no address moves after it.
    int grow_mask_arena(hipStream_t s) {
        const size_t words = mask_words(), table_bytes = (size_t)SA_MAX_TOKEN_MASKS * words * sizeof(uint32_t),
                     dyn_bytes = (size_t)c.max_slots * words * sizeof(uint32_t);
        Carve cv;
        const size_t o_slot = cv.take((size_t)c.max_slots * sizeof(int)), o_table = cv.take(table_bytes + dyn_bytes);
        DevBlock nb, &old = blk[B_MASK];
        int rc = nb.alloc(cv.off);
        if (rc) return rc;
        rc = (int)hipMemcpyAsync(nb.dev + o_slot, slot_mask, (size_t)c.max_slots * sizeof(int), hipMemcpyDeviceToDevice, s);
        if (!rc) rc = (int)hipMemcpyAsync(nb.dev + o_table, mask_table, table_bytes, hipMemcpyDeviceToDevice, s);
        if (!rc) rc = (int)hipDeviceSynchronize();          // the copies are done and nothing in flight reads the old block
        if (rc) { nb.release(); return rc; }
        drop_graphs();
        std::swap(nb.st, old.st);
        old.release();
        old = nb;
        slot_mask = reinterpret_cast<int*>(nb.dev + o_slot);
        mask_table = reinterpret_cast<uint32_t*>(nb.dev + o_table);
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
    int set_slot_lexicon(const int32_t* slots, const int32_t* states, int n, hipStream_t s) {
        const int *ds, *dt;
        const int rc = stage_slot_call(B_LEX_SLOTS, lex_states > 0, slots, {states}, n, s, [&](int i) { return states[i] >= -1 && states[i] < lex_states; }, &ds, &dt);
        if (rc || !ds) return rc;
        return launch_lexicon_start(lex_args(), ds, dt, n, s);
    }

    // The automaton of boosted decoding (boost.h), from host arrays. Everything is checked before anything is enqueued or allocated: the
    // kernels read the tables unchecked. New tables set every slot back to "not boosted".
    int set_boost(const int32_t* edge_off, const int32_t* edge_tok, const int32_t* edge_next, int n_states, int n_edges, int out_state,
                  int word_row, hipStream_t s) {
        if (n_states < 0 || n_states > SA_MAX_LEXICON_STATES || n_edges < 0 || n_edges > SA_MAX_LEXICON_EDGES) return SA_ERR_ARG;
        if (n_states == 0) return boost_off(s);
        if (!edge_off || (n_edges > 0 && (!edge_tok || !edge_next))) return SA_ERR_ARG;
        if (n_token_masks == 0 || excluded(M_BOOST)) return SA_ERR_STATE;
        if (!head2_ok() || cdiv(c.vocab, 64) > 4 * SA_HEAD_THREADS) return SA_ERR_STATE;      // the fallback head would have to run
        if (csr_check(edge_off, edge_tok, edge_next, n_states, n_edges, c.vocab) ||
            boost_check(edge_off, edge_tok, n_states, n_edges, out_state, word_row, n_token_masks, c.eos_token_id, c.pad_token_id))
            return SA_ERR_ARG;
        int rc;
        DevBlock& b = blk[B_BST_SLOTS];
        if (!b.dev) {                                       // first tables: the per-slot arrays (state and root -1, beta +inf), record B's partials, the outputs
            const size_t S = c.max_slots, out_b = (size_t)SA_MAX_STEPS * S * 4;
            Carve cv;
            const size_t o_state = cv.take(S * 4), o_root = cv.take(S * 4), o_beta = cv.take(S * 4),
                         o_amax = cv.take(S * (size_t)cdiv(c.vocab, 32) * sizeof(float4)), o_ptok = cv.take(out_b), o_pprob = cv.take(out_b);
            if ((rc = b.alloc(cv.off, 2 * out_b, S * 3 * sizeof(int) + 4096, {{o_state, o_beta - o_state, 0xffffffffu}, {o_beta, S * 4, 0x7f800000u}})))
                return rc;
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
    int set_slot_boost(const int32_t* slots, const int32_t* roots, const float* betas, int n, hipStream_t s) {
        const int *ds, *d[2];
        const int rc = stage_slot_call(B_BST_SLOTS, bst_states > 0, slots, {roots, betas}, n, s, [&](int i) {      // a boosted slot's beta: finite, >= 0 (NaN fails both)
            return roots[i] >= -1 && roots[i] < bst_states && (roots[i] < 0 || (betas[i] >= 0.f && betas[i] < INFINITY));
        }, &ds, d);
        if (rc || !ds) return rc;
        return launch_boost_start(bst_args(), ds, d[0], reinterpret_cast<const float*>(d[1]), n, s);
    }

    // Alternatives on / off. Memory on the first switch-on, or nothing (a failure leaves the handle as it was); switching drops captured
    // steps, which hold the other lm_head kernel and the head's null / non-null (max, total) pointer.
    int set_alternatives(int on) {
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
        DevBlock& b = blk[B_ALT];
        if (b.dev) return SA_OK;
        const size_t S = c.max_slots, cell = SA_MAX_ALTERNATIVES * 4, out_b = (size_t)SA_MAX_STEPS * S * cell;
        Carve cv;
        const size_t o_part = cv.take(S * (size_t)cdiv(c.vocab, 64) * SA_MAX_ALTERNATIVES * sizeof(float2)), o_bt = cv.take(S * sizeof(float2)),
                     o_tok = cv.take(out_b), o_prob = cv.take(out_b);
        const int rc = b.alloc(cv.off, 2 * out_b);
        if (rc) return rc;
        alt_part = reinterpret_cast<float2*>(b.dev + o_part);
        best_tot = reinterpret_cast<float2*>(b.dev + o_bt);
        alt_token = reinterpret_cast<int*>(b.dev + o_tok);
        alt_prob = reinterpret_cast<float*>(b.dev + o_prob);
        StepOutputs& o = outs[STEPS_ALTS];
        o.add(alt_token, cell); o.add(alt_prob, cell);
        o.host = b.host;
        return SA_OK;
    }

    // Beam search on (width 2..SA_MAX_BEAMS) / off (0). Memory on the first switch-on, or nothing (a failure leaves the handle as it was);
    // switching drops captured steps, which hold the other lm_head kernel, the fused or unfused head and no selection / fork launches.
    int set_beam(int width, int nop_id) {
        if (width != 0 && (width < 2 || width > SA_MAX_BEAMS || width > c.max_slots)) return SA_ERR_ARG;
        if (width && excluded(M_BEAM)) return SA_ERR_STATE;
        DevBlock& b = blk[B_BEAM];
        if (width) {
            int rc = ensure_alt_arena();
            if (rc) return rc;
            if (!b.dev) {
                const size_t S = c.max_slots, out_b = (size_t)SA_MAX_STEPS * S * 4;
                Carve cv;
                size_t o_slot[6], o_out[5];
                for (size_t& v : o_slot) v = cv.take(S * 4);
                for (size_t& v : o_out) v = cv.take(out_b);
                if ((rc = b.alloc(cv.off, 5 * out_b, 0, {{o_slot[3], S * 4, 0xffffffffu}}))) return rc;      // fork_src -1: nothing to copy
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

    // Forced decoding on / off. Memory on the first switch-on, or nothing (a failure leaves the handle as it was); switching drops captured
    // steps, which hold the other lm_head kernel and the head's empty / filled ForcedHead. Switch-off sets the table back to -1.
    int set_forced(int on) {
        if (on != 0 && on != 1) return SA_ERR_ARG;
        if (on && excluded(M_FORCED)) return SA_ERR_STATE;
        const size_t S = c.max_slots, table_bytes = S * SA_MAX_FORCED_TOKENS * sizeof(int), out_b = (size_t)SA_MAX_STEPS * S * 4;
        DevBlock& b = blk[B_FORCED];
        if (on && !b.dev) {
            Carve cv;
            const size_t o_table = cv.take(table_bytes), o_cursor = cv.take(S * sizeof(int)), o_flogit = cv.take(S * sizeof(float)),
                         o_gtok = cv.take(out_b), o_gprob = cv.take(out_b), o_logp = cv.take(out_b);
            const int rc = b.alloc(cv.off, 3 * out_b, table_bytes + (2 * S + 1) * sizeof(int) + 4096, {{o_table, table_bytes, 0xffffffffu}});   // every slot free-running
            if (rc) return rc;
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
    int set_forced_tokens(const int32_t* slots, const int32_t* tokens, const int32_t* offsets, int n, hipStream_t s) {
        if (n < 0 || n > c.max_slots) return SA_ERR_ARG;
        if (!forcing) return SA_ERR_STATE;
        if (n == 0) return SA_OK;
        if (offsets[0] < 0) return SA_ERR_ARG;
        if (check_slots(slots, n, c.max_slots, [&](int i) {
                const int len = offsets[i + 1] - offsets[i];
                if (len < 0 || len > SA_MAX_FORCED_TOKENS) return false;
                for (int j = offsets[i]; j < offsets[i + 1]; ++j)
                    if (tokens[j] < 0 || tokens[j] >= c.vocab) return false;
                return true;
            }))
            return SA_ERR_ARG;
        Stager& t = blk[B_FORCED].st;
        t.begin();
        const int* ds = t.put(slots, n);
        const int* dof = t.put(offsets, (size_t)n + 1);
        const int* dt = t.put(tokens + offsets[0], (size_t)(offsets[n] - offsets[0]));
        if (!ds || !dof || !dt) return SA_ERR_NOMEM;
        int rc = t.flush(s);
        if (rc) return rc;
        hipLaunchKernelGGL(set_forced_tokens_kernel, dim3(n), dim3(256), 0, s, ds, dt - offsets[0], dof, forced_table, forced_cursor,
                           SA_MAX_FORCED_TOKENS);
        return (int)hipGetLastError();
    }

    // ---------------------------------------------------------------------------------------- prompt store
    // The plain half of surya_rec_restore: everything about the entries and the fans is checked here, before anything is enqueued or
    // changed; then the host's length bounds, the staged lists (RestorePlan: device addresses) and every fan slot's kv_len. RecModel<T>
    // copies the rows and runs the head pass behind it.
    struct RestorePlan { const int *first, *lens, *foff, *fslots, *ffirst; int F; };
    int restore_plan(const int32_t* first, const int32_t* fan_offsets, const int32_t* fan_slots, int n, hipStream_t s, RestorePlan* p) {
        if (n > c.max_slots) return SA_ERR_ARG;
        if (kv8) return SA_ERR_STATE;                       // the store holds bf16 / fp16 / fp32 rows only
        // beam search owns whole groups and forks on its own: single-slot fans, lead slots of whole groups
        if (check_fans(fan_offsets, fan_slots, n, c.max_slots, [&](int i, int j) {
                return beam == 0 || (fan_offsets[i + 1] - fan_offsets[i] == 1 && fan_slots[j] % beam == 0 && fan_slots[j] + beam <= c.max_slots);
            }))
            return SA_ERR_ARG;
        for (int i = 0; i < n; ++i)
            if (!store_live.count(first[i])) return SA_ERR_ARG;
        const int F = fan_offsets[n];
        if (h_len.size() < (size_t)c.max_slots) h_len.resize(c.max_slots, 0);
        std::vector<int> lens(n), f_lens, f_first;
        for (int i = 0; i < n; ++i) {
            lens[i] = store_live[first[i]];
            for (int j = fan_offsets[i]; j < fan_offsets[i + 1]; ++j) {
                for (int b = 0; b < std::max(beam, 1); ++b) h_len[fan_slots[j] + b] = lens[i];
                f_lens.push_back(lens[i]); f_first.push_back(first[i]);
            }
        }
        st.begin();
        *p = RestorePlan{st.put(first, n), st.put(lens), st.put(fan_offsets, n + 1), st.put(fan_slots, F), nullptr, F};
        const int* d_flens = st.put(f_lens);
        p->ffirst = st.put(f_first);
        if (!p->first || !p->lens || !p->foff || !p->fslots || !d_flens || !p->ffirst) return SA_ERR_NOMEM;
        const int rc = st.flush(s);
        if (rc) return rc;
        hipLaunchKernelGGL(set_slot_state_kernel, dim3(cdiv(F, 256)), dim3(256), 0, s, p->fslots, d_flens, kv_len, F);
        return SA_OK;
    }
    int drop_prompts(const int32_t* first, int n) {
        std::set<int> named;
        for (int i = 0; i < n; ++i)
            if (!store_live.count(first[i]) || !named.insert(first[i]).second) return SA_ERR_ARG;
        for (int f : named) store_live.erase(f);
        return SA_OK;
    }
    int prompt_store_info(int32_t* cap_rows, int32_t* live_entries) {
        *cap_rows = store_cap; *live_entries = (int32_t)store_live.size();
        return SA_OK;
    }

    // --------------------------------------------------------------------------------------------- stepping
    int set_active(const int32_t* slots, int n, hipStream_t s) {
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
    int set_next_tokens(const int32_t* slots, const int32_t* toks, int n, hipStream_t s) {
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
    // What decode_async does behind its steps: the sets that are on go to the pinned mirror of ring half `ring`, behind an event.
    int mirror_steps(int n_steps, int ring, hipStream_t s) {
        for (int k = 0; k < STEPS_SETS; ++k) {
            outs[k].mirrored[ring] = false;                 // a set that is off mirrors nothing: wait_steps refuses this ring half
            const int rc = steps_on((StepSet)k) ? outs[k].mirror(ring, n_steps, s) : SA_OK;
            if (rc) return rc;
        }
        SA_HIP(hipEventRecord(ev_ring[ring], s));
        return SA_OK;
    }
    // The fields of one set for the steps read_outputs / wait_outputs return, same [step][slot] indexing. A set that is off is refused,
    // and so is a ring half whose decode_async was enqueued while the set was off.
    int wait_steps(StepSet set, int n_steps, int ring, std::initializer_list<void*> dst) {      // dst: one pointer per field of the set
        if (n_steps < 0 || n_steps > SA_MAX_STEPS / 2 || ring < 0 || ring > 1) return SA_ERR_ARG;
        if (!steps_on(set) || !outs[set].mirrored[ring]) return SA_ERR_STATE;
        SA_HIP(hipEventSynchronize(ev_ring[ring]));
        outs[set].wait(ring, n_steps, dst.begin());
        return SA_OK;
    }
    int read_steps(StepSet set, int n_steps, std::initializer_list<void*> dst, hipStream_t s) {
        if (n_steps <= 0 || n_steps > SA_MAX_STEPS) return SA_ERR_ARG;
        if (!steps_on(set)) return SA_ERR_STATE;
        return outs[set].read(n_steps, dst.begin(), s);
    }
};

}  // namespace sa
