// Prompt store (surya_rec_prefill_keep / surya_rec_restore): the KV rows of a prefilled prompt copied out of its slot into a store that
// outlives the slot, and landed again in as many slots as a later call asks for, with the launchers RecModel<T> and the
// surya_op_rec_kv_keep / surya_op_rec_kv_restore hooks share. The shape is kv_fanout_kernel's (kv_fanout.h): one read, K stores.
#pragma once
#include "common.h"

namespace sa {

// The store is [K | V][layer][kv_head][cap][D] (sk and sv are the two halves): the rows of one (K | V, layer, kv head) of an entry
// [first, first + len) are contiguous, as a (layer, slot, kv head) run of the cache [layer][slot][kv_head][Tmax][D] is. Rows are whole
// 16-byte units (the launchers check), so lane i moves unit i, four loads in flight per thread. Workgroup (n, layer * kv_heads + head,
// K | V); everything a workgroup leaves on is workgroup-uniform. len is clamped to [0, Tmax] and to cap - first; an entry whose first row
// or whose slot is out of range is skipped, so nothing outside the named runs is touched.
constexpr int SA_STORE_THREADS = 256;

struct StoreRun { int first, rows; };
__device__ inline StoreRun store_run(int first, int len, int Tmax, int cap) {      // rows == 0: nothing to move
    if (first < 0 || first >= cap) return StoreRun{0, 0};
    return StoreRun{first, min(min(max(len, 0), Tmax), cap - first)};
}

// Entry n: rows [0, len[n]) of slot[n] go to store rows [first[n], first[n] + len[n]). Where x is given, the (layer 0, head 0, K)
// workgroup of entry n also copies the hidden row x[last_row[n]] to hid[first[n]] ([cap][H], whole 16-byte units): the row the head pass
// of a later restore reads (a last_row outside [0, x_rows) copies none). No two entries of one launch may overlap in the store (surya_rec_prefill_keep checks).
template <typename T>
__global__ __launch_bounds__(SA_STORE_THREADS) void kv_keep_kernel(const T* __restrict__ kc, const T* __restrict__ vc, T* __restrict__ sk,
                                                                   T* __restrict__ sv, const int* __restrict__ slot, const int* __restrict__ first,
                                                                   const int* __restrict__ len, int n_slots, int nkv, int Tmax, int D, int cap,
                                                                   const T* __restrict__ x, const int* __restrict__ last_row, T* __restrict__ hid,
                                                                   int H, int x_rows) {
    const int n = blockIdx.x;
    const int src = slot[n];
    const StoreRun r = store_run(first[n], len[n], Tmax, cap);
    if (src < 0 || src >= n_slots || r.rows == 0) return;
    constexpr int V = 16 / (int)sizeof(T);
    constexpr int TH = SA_STORE_THREADS;
    if (x && blockIdx.y == 0 && blockIdx.z == 0 && last_row[n] >= 0 && last_row[n] < x_rows) {
        const uint4* hp = reinterpret_cast<const uint4*>(x + (long)last_row[n] * H);
        uint4* hq = reinterpret_cast<uint4*>(hid + (long)r.first * H);
        for (int u = threadIdx.x; u < H / V; u += TH) hq[u] = hp[u];
    }
    const int layer = blockIdx.y / nkv, head = blockIdx.y % nkv;
    const long run = (long)Tmax * D;
    const T* cache = blockIdx.z ? vc : kc;
    T* store = blockIdx.z ? sv : sk;
    const uint4* sp = reinterpret_cast<const uint4*>(cache + (((long)layer * n_slots + src) * nkv + head) * run);
    uint4* dp = reinterpret_cast<uint4*>(store + ((long)blockIdx.y * cap + r.first) * D);
    const int units = (int)(((long)r.rows * D) / V);
    int u = threadIdx.x;
    for (; u + 3 * TH < units; u += 4 * TH) {
        const uint4 v0 = sp[u], v1 = sp[u + TH], v2 = sp[u + 2 * TH], v3 = sp[u + 3 * TH];
        dp[u] = v0; dp[u + TH] = v1; dp[u + 2 * TH] = v2; dp[u + 3 * TH] = v3;
    }
    for (; u < units; u += TH) dp[u] = sp[u];
}

// Entry n: store rows [first[n], first[n] + len[n]) go to rows [0, len[n]) of every slot of fan_dst[fan_off[n] .. fan_off[n + 1]): read
// once, the same registers stored to every destination in turn. fan_off is clamped to [0, n_dst]; a destination out of range is skipped.
// No slot may be a destination twice in one launch (surya_rec_restore checks): then no workgroup writes what another writes.
template <typename T>
__global__ __launch_bounds__(SA_STORE_THREADS) void kv_restore_kernel(T* __restrict__ kc, T* __restrict__ vc, const T* __restrict__ sk,
                                                                      const T* __restrict__ sv, const int* __restrict__ first,
                                                                      const int* __restrict__ len, const int* __restrict__ fan_off,
                                                                      const int* __restrict__ fan_dst, int n_dst, int n_slots, int nkv, int Tmax,
                                                                      int D, int cap) {
    const int n = blockIdx.x;
    const StoreRun r = store_run(first[n], len[n], Tmax, cap);
    const int d0 = min(max(fan_off[n], 0), n_dst), d1 = min(max(fan_off[n + 1], 0), n_dst);
    if (d1 <= d0 || r.rows == 0) return;
    constexpr int V = 16 / (int)sizeof(T);
    constexpr int TH = SA_STORE_THREADS;
    const int layer = blockIdx.y / nkv, head = blockIdx.y % nkv;
    const long run = (long)Tmax * D;
    const long slot_stride = (long)nkv * run;
    T* cache = blockIdx.z ? vc : kc;
    const T* store = blockIdx.z ? sv : sk;
    T* lane0 = cache + ((long)layer * n_slots * nkv + head) * run;   // slot 0's run of this (layer, kv head)
    const uint4* sp = reinterpret_cast<const uint4*>(store + ((long)blockIdx.y * cap + r.first) * D);
    const int units = (int)(((long)r.rows * D) / V);
    int u = threadIdx.x;
    for (; u + 3 * TH < units; u += 4 * TH) {
        const uint4 v0 = sp[u], v1 = sp[u + TH], v2 = sp[u + 2 * TH], v3 = sp[u + 3 * TH];
        for (int j = d0; j < d1; ++j) {
            const int dst = fan_dst[j];
            if (dst < 0 || dst >= n_slots) continue;
            uint4* dp = reinterpret_cast<uint4*>(lane0 + dst * slot_stride);
            dp[u] = v0; dp[u + TH] = v1; dp[u + 2 * TH] = v2; dp[u + 3 * TH] = v3;
        }
    }
    for (; u < units; u += TH) {
        const uint4 v = sp[u];
        for (int j = d0; j < d1; ++j) {
            const int dst = fan_dst[j];
            if (dst < 0 || dst >= n_slots) continue;
            reinterpret_cast<uint4*>(lane0 + dst * slot_stride)[u] = v;
        }
    }
}

// The shape checks of both launches: launch_kv_fanout's, and a store whose runs stay below 2^31 units.
template <typename T>
int kv_store_shape(const void* kc, const void* vc, const void* sk, const void* sv, int layers, int n_slots, int nkv, int Tmax, int D, int cap) {
    if (!kc || !vc || !sk || !sv || layers <= 0 || n_slots <= 0 || nkv <= 0 || Tmax <= 0 || D <= 0 || cap <= 0) return SA_ERR_ARG;
    if ((D * sizeof(T)) % 16 || ((uintptr_t)kc | (uintptr_t)vc | (uintptr_t)sk | (uintptr_t)sv) % 16) return SA_ERR_SHAPE;
    if ((long)layers * nkv > 65535 || (long)Tmax * D > 0x7fffffffL) return SA_ERR_SHAPE;
    return SA_OK;
}

// n entries. x == nullptr: the KV rows only.
template <typename T>
int launch_kv_keep(const T* kc, const T* vc, T* sk, T* sv, const int* slot, const int* first, const int* len, int n, int layers, int n_slots,
                   int nkv, int Tmax, int D, int cap, const T* x, const int* last_row, T* hid, int H, int x_rows, hipStream_t s) {
    if (n <= 0) return n < 0 ? (int)SA_ERR_ARG : (int)SA_OK;
    if (!slot || !first || !len) return SA_ERR_ARG;
    if (const int rc = kv_store_shape<T>(kc, vc, sk, sv, layers, n_slots, nkv, Tmax, D, cap)) return rc;
    if (x && (!last_row || !hid || H <= 0)) return SA_ERR_ARG;
    if (x && ((H * sizeof(T)) % 16 || ((uintptr_t)x | (uintptr_t)hid) % 16)) return SA_ERR_SHAPE;
    hipLaunchKernelGGL(kv_keep_kernel<T>, dim3(n, layers * nkv, 2), dim3(SA_STORE_THREADS), 0, s, kc, vc, sk, sv, slot, first, len, n_slots, nkv, Tmax,
                       D, cap, x, last_row, hid, H, x_rows);
    return (int)hipGetLastError();
}

// n entries, n_dst entries of fan_dst in all.
template <typename T>
int launch_kv_restore(T* kc, T* vc, const T* sk, const T* sv, const int* first, const int* len, const int* fan_off, const int* fan_dst, int n,
                      int n_dst, int layers, int n_slots, int nkv, int Tmax, int D, int cap, hipStream_t s) {
    if (n <= 0 || n_dst <= 0) return n < 0 || n_dst < 0 ? (int)SA_ERR_ARG : (int)SA_OK;
    if (!first || !len || !fan_off || !fan_dst) return SA_ERR_ARG;
    if (const int rc = kv_store_shape<T>(kc, vc, sk, sv, layers, n_slots, nkv, Tmax, D, cap)) return rc;
    hipLaunchKernelGGL(kv_restore_kernel<T>, dim3(n, layers * nkv, 2), dim3(SA_STORE_THREADS), 0, s, kc, vc, sk, sv, first, len, fan_off, fan_dst,
                       n_dst, n_slots, nkv, Tmax, D, cap);
    return (int)hipGetLastError();
}

}  // namespace sa
