// Plain-C++ build of surya_amd/csrc/beam_core.h for tests/test_beam_cpu.py (g++ -ffp-contract=off): the selection and placement of any
// number of groups, group g at slots [g * B, g * B + B).
#include "../../surya_amd/csrc/beam_core.h"

extern "C" void beam_select_host(int n_groups, int B, const float* score, const int* fin, const int* alt_id, const float* alt_p, int eos, int pad,
                                 int nop, int first, int* token, int* parent, int* rank, int* finished, int* fork_src, float* prob, float* logp) {
    for (int g = 0; g < n_groups; ++g) {
        const int s0 = g * B;
        sa::beam::GroupOut o;
        sa::beam::select_group(B, s0, score + s0, fin + s0, alt_id + s0 * SA_BEAM_ALTS, alt_p + s0 * SA_BEAM_ALTS, eos, pad, nop, first, o);
        for (int b = 0; b < B; ++b) {
            token[s0 + b] = o.token[b]; parent[s0 + b] = o.parent[b]; rank[s0 + b] = o.rank[b]; finished[s0 + b] = o.finished[b];
            fork_src[s0 + b] = o.fork_src[b]; prob[s0 + b] = o.prob[b]; logp[s0 + b] = o.logp[b];
        }
    }
}
