// Prompt fan-out (surya_rec_prefill_shared): the KV rows of one prefilled slot copied to every other slot of its fan, with the launcher
// RecModel<T> and the surya_op_rec_kv_fanout hook share. kv_fork_kernel (beam.h) reads its source once per destination, which is right
// for the 0-3 moves of a beam step; a fan of 16-64 candidates reads its source ONCE here and stores it fan - 1 times.
#pragma once
#include "common.h"

namespace sa {

// Sequence n: rows [0, fan_len[n]) of every (layer, kv head) run of K and V go from slot fan_src[n] to the slots
// fan_dst[fan_off[n] .. fan_off[n + 1]). The cache is [layer][slot][kv_head][Tmax][D]: a (layer, slot, kv head) run is contiguous and its
// rows are whole 16-byte units (launch_kv_fanout checks), so lane i moves unit i: four loads in flight per thread, then the same four
// registers stored to every destination in turn. Workgroup (n, layer * kv_heads + head, K | V). Everything a workgroup leaves on is
// workgroup-uniform. fan_len is clamped to [0, Tmax], fan_off to [0, n_dst]; a destination out of range or equal to the source is skipped,
// so nothing outside the named runs is touched. No slot may be the source of one sequence and a destination of another, or a destination
// twice, in one launch (surya_rec_prefill_shared checks): then no workgroup reads or writes what another writes.
constexpr int SA_FANOUT_THREADS = 256;
template <typename T>
__global__ __launch_bounds__(SA_FANOUT_THREADS) void kv_fanout_kernel(T* __restrict__ kc, T* __restrict__ vc, const int* __restrict__ fan_src,
                                                                      const int* __restrict__ fan_off, const int* __restrict__ fan_dst,
                                                                      const int* __restrict__ fan_len, int n_dst, int n_slots, int nkv, int Tmax,
                                                                      int D) {
    const int n = blockIdx.x;
    const int src = fan_src[n];
    const int d0 = min(max(fan_off[n], 0), n_dst), d1 = min(max(fan_off[n + 1], 0), n_dst);
    const int rows = min(max(fan_len[n], 0), Tmax);
    if (src < 0 || src >= n_slots || d1 <= d0 || rows == 0) return;
    T* cache = blockIdx.z ? vc : kc;
    const long run = (long)Tmax * D;                                  // elements of one (layer, slot, kv head) run
    const long slot_stride = (long)nkv * run;
    const int layer = blockIdx.y / nkv, head = blockIdx.y % nkv;
    T* lane0 = cache + ((long)layer * n_slots * nkv + head) * run;   // slot 0's run of this (layer, kv head)
    constexpr int V = 16 / (int)sizeof(T);
    constexpr int TH = SA_FANOUT_THREADS;
    const uint4* sp = reinterpret_cast<const uint4*>(lane0 + src * slot_stride);
    const int units = (int)(((long)rows * D) / V);
    int u = threadIdx.x;
    for (; u + 3 * TH < units; u += 4 * TH) {
        const uint4 v0 = sp[u], v1 = sp[u + TH], v2 = sp[u + 2 * TH], v3 = sp[u + 3 * TH];
        for (int j = d0; j < d1; ++j) {
            const int dst = fan_dst[j];
            if (dst < 0 || dst >= n_slots || dst == src) continue;
            uint4* dp = reinterpret_cast<uint4*>(lane0 + dst * slot_stride);
            dp[u] = v0; dp[u + TH] = v1; dp[u + 2 * TH] = v2; dp[u + 3 * TH] = v3;
        }
    }
    for (; u < units; u += TH) {
        const uint4 v = sp[u];
        for (int j = d0; j < d1; ++j) {
            const int dst = fan_dst[j];
            if (dst < 0 || dst >= n_slots || dst == src) continue;
            reinterpret_cast<uint4*>(lane0 + dst * slot_stride)[u] = v;
        }
    }
}

// n_seqs sequences, n_dst entries of fan_dst in all. The shape checks are launch_kv_fork's.
template <typename T>
int launch_kv_fanout(T* kc, T* vc, const int* fan_src, const int* fan_off, const int* fan_dst, const int* fan_len, int n_seqs, int n_dst,
                     int layers, int n_slots, int nkv, int Tmax, int D, hipStream_t s) {
    if (n_seqs <= 0 || n_dst <= 0) return n_seqs < 0 || n_dst < 0 ? (int)SA_ERR_ARG : (int)SA_OK;
    if (!kc || !vc || !fan_src || !fan_off || !fan_dst || !fan_len || layers <= 0 || n_slots <= 0 || nkv <= 0 || Tmax <= 0 || D <= 0) return SA_ERR_ARG;
    if ((D * sizeof(T)) % 16 || ((uintptr_t)kc | (uintptr_t)vc) % 16) return SA_ERR_SHAPE;      // rows are whole 16-byte units at 16-byte addresses
    if ((long)layers * nkv > 65535 || (long)Tmax * D > 0x7fffffffL) return SA_ERR_SHAPE;
    hipLaunchKernelGGL(kv_fanout_kernel<T>, dim3(n_seqs, layers * nkv, 2), dim3(SA_FANOUT_THREADS), 0, s, kc, vc, fan_src, fan_off, fan_dst, fan_len,
                       n_dst, n_slots, nkv, Tmax, D);
    return (int)hipGetLastError();
}

}  // namespace sa
