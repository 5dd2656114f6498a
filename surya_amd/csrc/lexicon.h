// Lexicon-guided decoding (surya_rec_set_lexicon; recognition/lexicon.py compiles the tables): a line is exactly one entry of a word list.
// The automaton is sparse (CSR: a state's allowed set is its handful of children), far too large for one mask-table row per state, so every
// decoder slot owns ONE row of the mask table -- row id row_base + slot, behind the static rows -- and these two kernels rewrite it on the
// device: lexicon_start_kernel when a line is given its slot, lexicon_step_kernel behind the head of every step. The masked lm_head
// epilogues (TokenMask, gemm.h) then read the row like any static allowlist; none of them changes. Stream order does the rest: the lm_head
// of step k + 1 starts behind the step kernel of step k. Plain vector stores and vector atomics only.
//
// The launch code below is the only place that launches them: the engine (rec_engine.h) and the op hooks (surya_op_rec_lexicon_start /
// surya_op_rec_lexicon_step on caller-owned buffers) both go through it. The kernels read the tables unchecked: the engine validates them
// on the host (RecModel::set_lexicon), a caller of the op hooks answers for its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sa {

#define SA_LEXICON_START_THREADS 256
#define SA_LEXICON_STEP_THREADS 64      // one wave: a state has a handful of children; more are strided over

struct LexiconArgs {
    const int* edge_off = nullptr;      // [n_states + 1]
    const int* edge_tok = nullptr;      // [n_edges], strictly ascending inside a state, every id in [0, vocab)
    const int* edge_next = nullptr;     // [n_edges]
    const uint8_t* state_flags = nullptr;   // [n_states]: bit 0 terminal (eos and pad allowed), bit 1 the no-output token allowed
    uint32_t* table = nullptr;          // the mask table: rows of `words` words; slot s owns row row_base + s
    int words = 0, row_base = 0;
    int* slot_state = nullptr;          // [slots], -1 = no lexicon
    int* slot_mask = nullptr;           // [slots]
    int vocab = 0, eos_id = -1, pad_id = -1, nop_id = -1;   // eos / pad / nop outside [0, vocab) have no bit
};

// The allowed set of state `st`, applied to `row` by the whole workgroup: SET = atomicOr of every bit (children share words: a-z sit in
// two), !SET = 0 to every word that holds one of the bits (the row holds nothing but this set, so whole words are right).
template <bool SET>
__device__ __forceinline__ void lexicon_apply(const LexiconArgs& a, uint32_t* row, int st) {
    auto put = [&](int id) {
        if ((unsigned)id >= (unsigned)a.vocab) return;
        if (SET) atomicOr(&row[id >> 5], 1u << (id & 31));
        else row[id >> 5] = 0u;
    };
    const int e0 = a.edge_off[st], e1 = a.edge_off[st + 1];
    for (int e = e0 + (int)threadIdx.x; e < e1; e += (int)blockDim.x) put(a.edge_tok[e]);
    if (threadIdx.x == 0) {
        const int f = a.state_flags[st];
        if (f & 1) { put(a.eos_id); put(a.pad_id); }
        if (f & 2) put(a.nop_id);
    }
}

// Workgroup i: slot slots[i] starts in states[i]. -1 = no lexicon: the slot's state says so, its mask id and row are left alone. Else the
// whole row is zeroed (a previous occupant's bits may be anywhere), the start state's bits are set and the slot's mask id names the row.
static __global__ __launch_bounds__(SA_LEXICON_START_THREADS) void lexicon_start_kernel(LexiconArgs a, const int* __restrict__ slots,
                                                                                 const int* __restrict__ states) {
    const int slot = slots[blockIdx.x], st = states ? states[blockIdx.x] : -1;
    if (threadIdx.x == 0) a.slot_state[slot] = st;
    if (st < 0) return;                                       // (workgroup-uniform)
    uint32_t* row = a.table + (long)(a.row_base + slot) * a.words;
    for (int w = threadIdx.x; w < a.words; w += SA_LEXICON_START_THREADS) row[w] = 0u;
    __syncthreads();                                          // the zeros are in place before any bit is set
    lexicon_apply<true>(a, row, st);
    if (threadIdx.x == 0) a.slot_mask[slot] = a.row_base + slot;
}

// Workgroup r: row r of the step, slot row_slot[r], whose head just wrote out_token[slot]. A slot without a lexicon, a row that ended (eos /
// pad: it keeps its state and row), an id outside the vocabulary (the head's "no column" index) and an id the state has no edge for (the
// mask makes that impossible but for the no-output token at a start state) touch nothing. Else: clear the old state's words, barrier --
// the old and the new set commonly share words --, set the new state's bits, store the state.
static __global__ __launch_bounds__(SA_LEXICON_STEP_THREADS) void lexicon_step_kernel(LexiconArgs a, const int* __restrict__ row_slot,
                                                                               const int* __restrict__ out_token) {
    const int slot = row_slot[blockIdx.x], st = a.slot_state[slot];
    if (st < 0) return;                                       // (every exit before the barrier is workgroup-uniform)
    const int t = out_token[slot];
    if (t == a.eos_id || t == a.pad_id || (unsigned)t >= (unsigned)a.vocab) return;
    int lo = a.edge_off[st], hi = a.edge_off[st + 1];         // binary search, every lane the same one
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a.edge_tok[mid] < t) lo = mid + 1; else hi = mid;
    }
    if (lo >= a.edge_off[st + 1] || a.edge_tok[lo] != t) return;
    const int ns = a.edge_next[lo];
    uint32_t* row = a.table + (long)(a.row_base + slot) * a.words;
    lexicon_apply<false>(a, row, st);
    __syncthreads();
    lexicon_apply<true>(a, row, ns);
    if (threadIdx.x == 0) a.slot_state[slot] = ns;
}

inline int launch_lexicon_start(const LexiconArgs& a, const int* slots, const int* states, int n, hipStream_t s) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(lexicon_start_kernel, dim3(n), dim3(SA_LEXICON_START_THREADS), 0, s, a, slots, states);
    return (int)hipGetLastError();
}
inline int launch_lexicon_step(const LexiconArgs& a, const int* row_slot, const int* out_token, int rows, hipStream_t s) {
    if (rows <= 0) return 0;
    hipLaunchKernelGGL(lexicon_step_kernel, dim3(rows), dim3(SA_LEXICON_STEP_THREADS), 0, s, a, row_slot, out_token);
    return (int)hipGetLastError();
}

}  // namespace sa
