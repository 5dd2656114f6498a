// Plain-C++ build of surya_amd/csrc/automaton_core.h for tests/test_automaton_cpu.py: the checks RecModel::set_lexicon and
// RecModel::set_boost run on their tables, in the engine's order (the structure first, then the feature's own rules).
#include "../../surya_amd/csrc/automaton_core.h"

extern "C" int csr_check_host(const int32_t* edge_off, const int32_t* edge_tok, const int32_t* edge_next, int n_states, int n_edges, int vocab) {
    return sa::csr_check(edge_off, edge_tok, edge_next, n_states, n_edges, vocab);
}

extern "C" int lexicon_tables_check_host(const int32_t* edge_off, const int32_t* edge_tok, const int32_t* edge_next, const uint8_t* flags,
                                         int n_states, int n_edges, int vocab, int eos, int pad, int nop) {
    const int rc = sa::csr_check(edge_off, edge_tok, edge_next, n_states, n_edges, vocab);
    return rc ? rc : sa::lexicon_check(edge_off, flags, n_states, vocab, eos, pad, nop);
}

extern "C" int boost_tables_check_host(const int32_t* edge_off, const int32_t* edge_tok, const int32_t* edge_next, int n_states, int n_edges,
                                       int vocab, int out_state, int word_row, int n_rows, int eos, int pad) {
    const int rc = sa::csr_check(edge_off, edge_tok, edge_next, n_states, n_edges, vocab);
    return rc ? rc : sa::boost_check(edge_off, edge_tok, n_states, n_edges, out_state, word_row, n_rows, eos, pad);
}
