// Lexicon-guided decoding (surya_rec_set_lexicon; recognition/lexicon.py compiles the tables): a line is exactly one entry of a word list.
// The automaton is sparse (CSR: a state's allowed set is its handful of children), far too large for one mask-table row per state, so every
// decoder slot owns ONE row of the mask table -- row id row_base + slot, behind the static rows -- and these two kernels rewrite it on the
// device: automaton_start_kernel when a line is given its slot, automaton_step_kernel behind the head of every step. The masked lm_head
// epilogues (TokenMask, gemm.h) then read the row like any static allowlist; none of them changes. Stream order does the rest: the lm_head
// of step k + 1 starts behind the step kernel of step k. Plain vector stores and vector atomics only.
//
// The launch code below is the only place that launches them: the engine (rec_engine.h) and the op hooks (surya_op_rec_lexicon_start /
// surya_op_rec_lexicon_step on caller-owned buffers) both go through it. The kernels read the tables unchecked: the engine validates them
// on the host (automaton_core.h), a caller of the op hooks answers for its own. Boosted decoding (boost.h) runs the same two kernels with
// TOTAL = true: an automaton in which a token without an edge takes a fallback transition.
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

// What the total automaton of boosted decoding (boost.h) takes beside LexiconArgs; the kernels ignore it when !TOTAL.
struct TotalOps {
    int* slot_root = nullptr;           // [slots]: the root state of the slot's list, -1 = not boosted
    float* slot_beta = nullptr;         // [slots]: the boost in logit units, +inf = not boosted
    int out_state = 0;                  // the shared state without edges
    int word_row = 0;                   // row of the mask table that holds the word-unit set
};

// Workgroup i: slot slots[i] starts in states[i]; TOTAL: that state is also the slot's root, betas[i] its boost. -1 (or states ==
// nullptr) = follows no automaton: the slot's state says so (TOTAL: and its root; beta +inf), its mask id and row are left alone. Else
// the whole row is zeroed (a previous occupant's bits may be anywhere), the start state's bits are set and the slot's mask id names the
// row. The operands are kernel arguments of their own, not members of one struct: a reference into a by-value struct argument costs
// lexicon_apply's lambdas scratch.
template <bool TOTAL>
static __global__ __launch_bounds__(SA_LEXICON_START_THREADS) void automaton_start_kernel(LexiconArgs a, TotalOps x, const int* __restrict__ slots,
                                                                                   const int* __restrict__ states,
                                                                                   const float* __restrict__ betas) {
    const int slot = slots[blockIdx.x], st = states ? states[blockIdx.x] : -1;
    if (threadIdx.x == 0) {
        a.slot_state[slot] = st;
        if (TOTAL) {
            x.slot_root[slot] = st;
            x.slot_beta[slot] = st < 0 ? INFINITY : betas[blockIdx.x];
        }
    }
    if (st < 0) return;                                       // (workgroup-uniform)
    uint32_t* row = a.table + (long)(a.row_base + slot) * a.words;
    for (int w = threadIdx.x; w < a.words; w += SA_LEXICON_START_THREADS) row[w] = 0u;
    __syncthreads();                                          // the zeros are in place before any bit is set
    lexicon_apply<true>(a, row, st);
    if (threadIdx.x == 0) a.slot_mask[slot] = a.row_base + slot;
}

// Workgroup r: row r of the step, slot row_slot[r], whose head just wrote out_token[slot]. A slot that follows no automaton, a row that
// ended (eos / pad: it keeps its state and row) and an id outside the vocabulary (the head's "no column" index) touch nothing. The next
// state is the edge's target. Without an edge: !TOTAL touches nothing (the mask makes that impossible but for the no-output token at a
// start state); TOTAL takes the fallback -- the shared out_state for a word unit, the slot's root for a boundary. A state that stays
// rewrites nothing: the row holds exactly that state's set, so clearing and setting it again would write the words that are there.
// Else: clear the old state's words, barrier -- the old and the new set commonly share words --, set the new state's bits, store the
// state. Sets may be empty when TOTAL.
template <bool TOTAL>
static __global__ __launch_bounds__(SA_LEXICON_STEP_THREADS) void automaton_step_kernel(LexiconArgs a, TotalOps x, const int* __restrict__ row_slot,
                                                                                 const int* __restrict__ out_token) {
    const int slot = row_slot[blockIdx.x], st = a.slot_state[slot];
    if (st < 0) return;                                       // (every exit before the barrier is workgroup-uniform)
    const int t = out_token[slot];
    if (t == a.eos_id || t == a.pad_id || (unsigned)t >= (unsigned)a.vocab) return;
    const int e1 = a.edge_off[st + 1];
    int lo = a.edge_off[st], hi = e1;                         // binary search, every lane the same one
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a.edge_tok[mid] < t) lo = mid + 1; else hi = mid;
    }
    int ns;
    if (lo < e1 && a.edge_tok[lo] == t) {
        ns = a.edge_next[lo];
    } else if (TOTAL) {
        const uint32_t w = a.table[(long)x.word_row * a.words + (t >> 5)];
        ns = (w >> (t & 31)) & 1u ? x.out_state : x.slot_root[slot];
    } else {
        return;
    }
    if (ns == st) return;
    uint32_t* row = a.table + (long)(a.row_base + slot) * a.words;
    lexicon_apply<false>(a, row, st);
    __syncthreads();
    lexicon_apply<true>(a, row, ns);
    if (threadIdx.x == 0) a.slot_state[slot] = ns;
}

template <bool TOTAL>
int launch_automaton_start(const LexiconArgs& a, const TotalOps& x, const int* slots, const int* states, const float* betas, int n,
                           hipStream_t s) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(automaton_start_kernel<TOTAL>, dim3(n), dim3(SA_LEXICON_START_THREADS), 0, s, a, x, slots, states, betas);
    return (int)hipGetLastError();
}
template <bool TOTAL>
int launch_automaton_step(const LexiconArgs& a, const TotalOps& x, const int* row_slot, const int* out_token, int rows, hipStream_t s) {
    if (rows <= 0) return 0;
    hipLaunchKernelGGL(automaton_step_kernel<TOTAL>, dim3(rows), dim3(SA_LEXICON_STEP_THREADS), 0, s, a, x, row_slot, out_token);
    return (int)hipGetLastError();
}
inline int launch_lexicon_start(const LexiconArgs& a, const int* slots, const int* states, int n, hipStream_t s) {
    return launch_automaton_start<false>(a, TotalOps{}, slots, states, nullptr, n, s);
}
inline int launch_lexicon_step(const LexiconArgs& a, const int* row_slot, const int* out_token, int rows, hipStream_t s) {
    return launch_automaton_step<false>(a, TotalOps{}, row_slot, out_token, rows, s);
}

}  // namespace sa
