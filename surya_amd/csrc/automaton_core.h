// The host-side checks of a sparse automaton in CSR form (edge_off / edge_tok / edge_next), shared by RecBase::set_lexicon and
// RecBase::set_boost (rec_state.h) and a plain-C++ build used by the CPU tests (tests/native/automaton_host.cpp). The kernels of
// lexicon.h and boost.h read the tables unchecked: these functions are what keeps a bad table from a stray read on the device. No HIP
// here. Every function returns SA_OK or SA_ERR_ARG and reads nothing outside the ranges it has already checked; the callers have
// checked the counts (>= 0, n_states >= 1) and the pointers.
#pragma once
#include <stdint.h>

#ifndef SA_OK                           // (include/surya_amd.h, restated so that this header stands alone)
#define SA_OK 0
#define SA_ERR_ARG (-1)
#endif

namespace sa {

// The structure both automata share: edge_off runs from 0 to n_edges without a step back, a state's tokens lie in [0, vocab) and
// ascend strictly (the step kernels search them), every target is a state.
inline int csr_check(const int32_t* edge_off, const int32_t* edge_tok, const int32_t* edge_next, int n_states, int n_edges, int vocab) {
    if (edge_off[0] != 0 || edge_off[n_states] != n_edges) return SA_ERR_ARG;
    for (int st = 0; st < n_states; ++st) {
        const int a = edge_off[st], b = edge_off[st + 1];
        if (a < 0 || b < a || b > n_edges) return SA_ERR_ARG;
        for (int e = a; e < b; ++e) {
            if (edge_tok[e] < 0 || edge_tok[e] >= vocab || edge_next[e] < 0 || edge_next[e] >= n_states) return SA_ERR_ARG;
            if (e > a && edge_tok[e] <= edge_tok[e - 1]) return SA_ERR_ARG;
        }
    }
    return SA_OK;
}

// The lexicon's own rules: flag bits 0 (terminal: eos and pad allowed) and 1 (the no-output token allowed) only; bit 1 needs `nop` in
// the vocabulary; every state has an allowed id -- a row without one would make the head emit the "no column" index.
inline int lexicon_check(const int32_t* edge_off, const uint8_t* flags, int n_states, int vocab, int eos, int pad, int nop) {
    const bool ends = (eos >= 0 && eos < vocab) || (pad >= 0 && pad < vocab);
    for (int st = 0; st < n_states; ++st) {
        const int f = flags[st];
        if (f & ~3) return SA_ERR_ARG;
        if ((f & 2) && (nop < 0 || nop >= vocab)) return SA_ERR_ARG;
        if (edge_off[st + 1] == edge_off[st] && !((f & 1) && ends) && !(f & 2)) return SA_ERR_ARG;
    }
    return SA_OK;
}

// The boost's own rules: out_state is a state without edges, word_row a row of the mask table (n_rows rows), and eos / pad are never
// preferred (the step kernel keeps the state behind them).
inline int boost_check(const int32_t* edge_off, const int32_t* edge_tok, int n_states, int n_edges, int out_state, int word_row, int n_rows,
                       int eos, int pad) {
    if (out_state < 0 || out_state >= n_states || word_row < 0 || word_row >= n_rows) return SA_ERR_ARG;
    if (edge_off[out_state + 1] != edge_off[out_state]) return SA_ERR_ARG;
    for (int e = 0; e < n_edges; ++e)
        if (edge_tok[e] == eos || edge_tok[e] == pad) return SA_ERR_ARG;
    return SA_OK;
}

}  // namespace sa
