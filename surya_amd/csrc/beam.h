// Beam search on the device (surya_rec_set_beam): the selection step behind topk_combine_kernel and the KV fork behind it, with the
// launchers RecModel<T> and the surya_op_rec_beam_select / surya_op_rec_kv_fork hooks share. The rules are beam_core.h's.
#pragma once
#include "beam_core.h"
#include "common.h"

namespace sa {

// One group = `width` consecutive slots from lead_list[g * stride] (stride 1: a list of lead slots, the prefill; stride = width: an active
// list of whole groups). State per slot, read and written: score, finished. Of the step, per slot: alt_token / alt_prob [slot][4] in, the
// five o_* arrays out. For the launches that follow: next_token (pad for a finished beam), fork_src / fork_base / fork_len (kv_fork_kernel).
// kv_len != nullptr: the engine's slot lengths -- the first selection gives every slot of the group the lead's length and records it as the
// group's prompt length; fork_len is the lead's length, fork_base the prompt length, or 0 on the first selection and for a destination
// whose beam was empty (it never received the prompt). kv_len == nullptr (a selection alone): fork_base / fork_len are not written.
struct BeamSelectArgs {
    const int* lead_list; int stride, n_groups, width, n_slots;
    const int* alt_token; const float* alt_prob;
    float* score; int* finished;
    int eos, pad, nop, first;
    int *o_token, *o_parent, *o_rank; float *o_prob, *o_logp;
    int *next_token, *fork_src;
    int *kv_len, *prompt_len, *fork_base, *fork_len; int Tmax;
};

static __global__ __launch_bounds__(64) void beam_select_kernel(BeamSelectArgs a) {
    const int g = blockIdx.x, lane = threadIdx.x, B = a.width;
    const int slot0 = a.lead_list ? a.lead_list[g * a.stride] : g * B;
    if (slot0 < 0 || slot0 + B > a.n_slots) return;                   // (wave-uniform) a list that names no whole group: nothing is touched
    __shared__ float s_score[SA_BEAM_MAX], s_p[SA_BEAM_MAX * SA_BEAM_ALTS];
    __shared__ int s_fin[SA_BEAM_MAX], s_id[SA_BEAM_MAX * SA_BEAM_ALTS];
    __shared__ beam::GroupOut s_out;
    if (lane < B * SA_BEAM_ALTS) {
        s_id[lane] = a.alt_token[slot0 * SA_BEAM_ALTS + lane];
        s_p[lane] = a.alt_prob[slot0 * SA_BEAM_ALTS + lane];
    }
    if (lane < B) {
        s_score[lane] = a.first ? 0.f : a.score[slot0 + lane];
        s_fin[lane] = a.first ? 0 : a.finished[slot0 + lane];
    }
    __syncthreads();
    if (lane == 0) beam::select_group(B, slot0, s_score, s_fin, s_id, s_p, a.eos, a.pad, a.nop, a.first, s_out);
    __syncthreads();
    if (lane < B) {
        const int slot = slot0 + lane;
        const bool was_empty = a.first || (s_fin[lane] && !(s_score[lane] > -INFINITY));
        a.o_token[slot] = s_out.token[lane];
        a.o_parent[slot] = s_out.parent[lane];
        a.o_rank[slot] = s_out.rank[lane];
        a.o_prob[slot] = s_out.prob[lane];
        a.o_logp[slot] = s_out.logp[lane];
        a.score[slot] = s_out.logp[lane];
        a.finished[slot] = s_out.finished[lane];
        a.next_token[slot] = s_out.finished[lane] ? a.pad : s_out.token[lane];
        a.fork_src[slot] = s_out.fork_src[lane];
        if (a.kv_len) {
            const int len = a.kv_len[slot0];                          // all slots of a group have the lead's length
            if (a.first) { a.kv_len[slot] = len; a.prompt_len[slot] = len; }
            a.fork_base[slot] = was_empty ? 0 : a.prompt_len[slot];
            a.fork_len[slot] = min(len, a.Tmax);
        }
    }
}

inline int launch_beam_select(const BeamSelectArgs& a, hipStream_t s) {
    if (a.n_groups <= 0) return SA_OK;
    if (a.width < 2 || a.width > SA_BEAM_MAX || a.stride < 1 || a.n_slots < a.width) return SA_ERR_ARG;
    if (!a.alt_token || !a.alt_prob || !a.score || !a.finished || !a.o_token || !a.o_parent || !a.o_rank || !a.o_prob || !a.o_logp ||
        !a.next_token || !a.fork_src)
        return SA_ERR_ARG;
    if (a.kv_len && (!a.prompt_len || !a.fork_base || !a.fork_len || a.Tmax <= 0)) return SA_ERR_ARG;
    hipLaunchKernelGGL(beam_select_kernel, dim3(a.n_groups), dim3(64), 0, s, a);
    return (int)hipGetLastError();
}

// KV fork: for every destination slot with fork_src >= 0, rows [base, len) of every (layer, kv head) of K and V are copied from the source
// slot's run to the destination's. The cache is [layer][slot][kv_head][Tmax][D]: a (layer, slot, kv head) run is contiguous and its rows are
// whole 16-byte units (launch_kv_fork checks), so lane i moves unit i of the range: 1 KiB per wave instruction, four in flight per thread.
// Workgroup (r, layer * kv_heads + head, K | V); destination slot = list ? list[r / per] + r % per : r (per = 1: the active list; per = width:
// a list of lead slots). fork_src / base / len are indexed by destination slot; a source is never a destination of the same step
// (beam_core.h), so no workgroup reads what another writes. base and len are clamped to [0, Tmax]: nothing outside the two runs is touched.
constexpr int SA_FORK_THREADS = 256;
template <typename T>
__global__ __launch_bounds__(SA_FORK_THREADS) void kv_fork_kernel(T* __restrict__ kc, T* __restrict__ vc, const int* __restrict__ list, int per,
                                                                  const int* __restrict__ fork_src, const int* __restrict__ base,
                                                                  const int* __restrict__ len, int n_slots, int nkv, int Tmax, int D) {
    const int r = blockIdx.x;
    const int dst = list ? list[r / per] + r % per : r;
    if (dst < 0 || dst >= n_slots) return;
    const int src = fork_src[dst];
    if (src < 0 || src >= n_slots || src == dst) return;
    const int r0 = max(base[dst], 0), r1 = min(len[dst], Tmax);
    if (r1 <= r0) return;
    T* cache = blockIdx.z ? vc : kc;
    const long run = (long)Tmax * D;                                  // elements of one (layer, slot, kv head) run
    const int layer = blockIdx.y / nkv, head = blockIdx.y % nkv;
    const long so = (((long)layer * n_slots + src) * nkv + head) * run, dof = (((long)layer * n_slots + dst) * nkv + head) * run;
    constexpr int V = 16 / (int)sizeof(T);
    const uint4* sp = reinterpret_cast<const uint4*>(cache + so + (long)r0 * D);
    uint4* dp = reinterpret_cast<uint4*>(cache + dof + (long)r0 * D);
    const int units = (int)(((long)(r1 - r0) * D) / V);
    int u = threadIdx.x;
    for (; u + 3 * SA_FORK_THREADS < units; u += 4 * SA_FORK_THREADS) {
        const uint4 v0 = sp[u], v1 = sp[u + SA_FORK_THREADS], v2 = sp[u + 2 * SA_FORK_THREADS], v3 = sp[u + 3 * SA_FORK_THREADS];
        dp[u] = v0; dp[u + SA_FORK_THREADS] = v1; dp[u + 2 * SA_FORK_THREADS] = v2; dp[u + 3 * SA_FORK_THREADS] = v3;
    }
    for (; u < units; u += SA_FORK_THREADS) dp[u] = sp[u];
}

template <typename T>
int launch_kv_fork(T* kc, T* vc, const int* list, int per, const int* fork_src, const int* base, const int* len, int rows, int layers, int n_slots,
                   int nkv, int Tmax, int D, hipStream_t s) {
    if (rows <= 0) return SA_OK;
    if (!kc || !vc || !fork_src || !base || !len || per < 1 || layers <= 0 || n_slots <= 0 || nkv <= 0 || Tmax <= 0 || D <= 0) return SA_ERR_ARG;
    if ((D * sizeof(T)) % 16 || ((uintptr_t)kc | (uintptr_t)vc) % 16) return SA_ERR_SHAPE;      // rows are whole 16-byte units at 16-byte addresses
    if ((long)layers * nkv > 65535 || (long)Tmax * D > 0x7fffffffL) return SA_ERR_SHAPE;
    hipLaunchKernelGGL(kv_fork_kernel<T>, dim3(rows, layers * nkv, 2), dim3(SA_FORK_THREADS), 0, s, kc, vc, list, per, fork_src, base, len, n_slots,
                       nkv, Tmax, D);
    return (int)hipGetLastError();
}

}  // namespace sa
