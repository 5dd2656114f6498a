// Beam search: selection and placement for ONE group of B beams, shared by beam_select_kernel (beam.h) and a plain-C++ build used by the
// CPU tests (tests/native/beam_host.cpp). No launch or memory-model code: plain arrays in, plain arrays out. This is the single statement
// of the rules (surya_rec_set_beam, include/surya_amd.h).
//
// A group owns B consecutive slots; beam b sits in slot b of the group. Inputs per beam: its cumulative score, its finished flag and the
// SA_BEAM_ALTS alternatives of this step (ids and probabilities, best first, id -1 / probability 0 = no such entry).
//   candidates   a live beam offers one candidate per alternative with id >= 0 and probability > 0, score = cum + log p; a finished beam
//                with a score above -inf offers itself, frozen, with its score unchanged (rank 0); a finished beam at -inf is an empty
//                beam and offers nothing. `first`: only beam 0 -- the lead slot, the only one prefilled -- offers candidates, from score 0.
//   log p        the fp32 logarithm as float(log(double(p))): the correctly rounded value, so the device and the host agree bit for bit
//                (the two logf implementations differ in the last place). The sum cum + log p is one fp32 addition.
//   selection    the best B candidates in the order score descending, parent slot ascending, rank ascending.
//   finished     a chosen token that is eos or pad finishes its beam; on the first selection the no-output id does too. A frozen beam
//                stays finished: token = pad, probability 0.
//   placement    for each parent, in slot order, its first chosen child (in selection order: alternatives come best first, so that is rank
//                order) stays in the parent's slot: parent = own index, no copy. Every further chosen child goes to a slot whose beam did not
//                survive, those slots ascending, the children parent by parent in selection order: parent = the source's index, fork_src =
//                its absolute slot. A source slot is a survivor, a destination is not: no fork reads what another fork of the step writes.
//   empty        slots left over (fewer than B candidates): token pad, parent -1, rank 0, probability 0, score -inf, finished.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef SA_HD
#if defined(__HIPCC__)
#define SA_HD __host__ __device__ __forceinline__
#else
#define SA_HD inline
#endif
#endif

#define SA_BEAM_MAX 4       // == SA_MAX_BEAMS (include/surya_amd.h)
#define SA_BEAM_ALTS 4      // == SA_MAX_ALTERNATIVES: the candidates a row reports

namespace sa {
namespace beam {

struct GroupOut {           // per slot of the group
    int token[SA_BEAM_MAX], parent[SA_BEAM_MAX], rank[SA_BEAM_MAX], finished[SA_BEAM_MAX], fork_src[SA_BEAM_MAX];
    float prob[SA_BEAM_MAX], logp[SA_BEAM_MAX];
};

SA_HD float log_prob(float p) { return (float)log((double)p); }

// score / fin [B]; alt_id / alt_p [B][SA_BEAM_ALTS]; slot0: the absolute slot of beam 0 (only fork_src uses it)
SA_HD void select_group(int B, int slot0, const float* score, const int* fin, const int* alt_id, const float* alt_p, int eos, int pad, int nop,
                        int first, GroupOut& o) {
    constexpr int NC = SA_BEAM_MAX * SA_BEAM_ALTS;
    float cs[NC];
    int cpar[NC], crank[NC], n = 0;
    for (int b = 0; b < (first ? 1 : B); ++b) {
        if (!first && fin[b]) {
            if (score[b] > -INFINITY) { cs[n] = score[b]; cpar[n] = b; crank[n] = -1; ++n; }      // frozen (rank -1 marks it here)
            continue;
        }
        const float cum = first ? 0.f : score[b];
        for (int j = 0; j < SA_BEAM_ALTS; ++j) {
            const float p = alt_p[b * SA_BEAM_ALTS + j];
            if (alt_id[b * SA_BEAM_ALTS + j] < 0 || !(p > 0.f)) continue;
            cs[n] = cum + log_prob(p); cpar[n] = b; crank[n] = j; ++n;
        }
    }
    // candidates were generated parent ascending, rank ascending: the first maximum of the rest is the next in selection order
    int sel[SA_BEAM_MAX], ns = 0;
    bool used[NC];
    for (int i = 0; i < NC; ++i) used[i] = false;
    for (; ns < B && ns < n; ++ns) {
        int bi = -1;
        for (int i = 0; i < n; ++i)
            if (!used[i] && (bi < 0 || cs[i] > cs[bi])) bi = i;
        used[bi] = true;
        sel[ns] = bi;
    }
    int cand_at[SA_BEAM_MAX], src_of[SA_BEAM_MAX];      // per slot: the candidate placed there (-1 = none yet), the slot it came from
    for (int b = 0; b < B; ++b) { cand_at[b] = -1; src_of[b] = -1; }
    bool placed[SA_BEAM_MAX];
    for (int k = 0; k < ns; ++k) {                      // first chosen child of every parent: in place
        const int par = cpar[sel[k]];
        placed[k] = cand_at[par] < 0;
        if (placed[k]) { cand_at[par] = sel[k]; src_of[par] = par; }
    }
    // the filled slots are now exactly the survivors; further children fill the others from the left, so a filled slot is never a source
    // that is written: sources are survivors, and those were all filled before this loop
    int free_at = 0;
    for (int par = 0; par < B; ++par)
        for (int k = 0; k < ns; ++k) {
            if (placed[k] || cpar[sel[k]] != par) continue;
            while (free_at < B - 1 && cand_at[free_at] >= 0) ++free_at;        // (there is one: distinct parents + further children <= B)
            cand_at[free_at] = sel[k]; src_of[free_at] = par;
            placed[k] = true;
        }
    for (int b = 0; b < B; ++b) {
        const int ci = cand_at[b];
        if (ci < 0) {
            o.token[b] = pad; o.parent[b] = -1; o.rank[b] = 0; o.prob[b] = 0.f; o.logp[b] = -INFINITY; o.finished[b] = 1; o.fork_src[b] = -1;
            continue;
        }
        const int par = cpar[ci], rk = crank[ci];
        o.parent[b] = par;
        o.logp[b] = cs[ci];
        o.fork_src[b] = par == b ? -1 : slot0 + par;
        if (rk < 0) {
            o.token[b] = pad; o.rank[b] = 0; o.prob[b] = 0.f; o.finished[b] = 1;
        } else {
            const int t = alt_id[par * SA_BEAM_ALTS + rk];
            o.token[b] = t; o.rank[b] = rk; o.prob[b] = alt_p[par * SA_BEAM_ALTS + rk];
            o.finished[b] = (t == eos || t == pad || (first && t == nop)) ? 1 : 0;
        }
    }
}

}  // namespace beam
}  // namespace sa
