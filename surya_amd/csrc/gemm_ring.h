// Loader / consumer LDS ring for the decode-regime 16-bit (bf16 / fp16) GEMMs (128 < M <= 256): gate|up (EPI_SWIGLU) and the split-K projections.
//
// The tiles of gemm_nt_kernel make every wave both load and multiply, and all waves meet at a workgroup barrier per K-tile. At one
// workgroup per CU that loop takes in ~28-35 GB/s per CU; here the roles are split:
//   * NL loader waves only issue global_load_lds_dwordx4 for the X and W rows of a K-tile into one slot of a SLOTS-deep ring, keep two
//     K-tiles in flight, and publish a slot behind a counted `s_waitcnt vmcnt` (each loader its own FULL word per slot);
//   * CWM x CWN consumer waves wait for the slot's FULL words, read all fragments of the K-tile into registers, release the slot (their
//     own FREE word per slot) after `lgkmcnt(0)` and only then issue the MFMAs.
// No workgroup barrier inside the K loop. The words are sequence numbers (fills / releases of a slot so far), so nothing is reset. They
// live in the same dynamic LDS array as the ring, and every access to them is inline asm that carries its own wait: hipcc neither drains
// vmcnt in front of them (the loaders' requests stay in flight) nor reorders them (memory clobbers). Every spin is bounded; a wave that
// gives up sets ring_error_word and stops waiting for the rest of the launch (wrong numbers, no hang); the host reads the word through
// ring_error().
//
// Arithmetic is gemm_nt_kernel's: the same LDS image (128-byte K-rows, XOR swizzle on the source address), the same v_mfma_f32_32x32x16_bf16 (_f16)
// with the weight fragment first, K walked K-tile by K-tile and kk = 0..3 inside one, split-K slices from the same kt_begin / kt_end
// formula. Each output element therefore sees the same MFMA sequence as on any other tile shape: results are bit-identical.
#pragma once

namespace sa {

static __device__ unsigned ring_error_word;     // != 0: some ring wave gave up waiting (one copy per translation unit: surya_gemm_ring_status asks each)

// (consumer waves, loader waves, slots): gate|up on 64 x 160 tiles -- 4 row blocks x 64 column blocks = 256 workgroups, one per CU, the four
// row blocks of a weight slab on one XCD -- and the split-K projections on the 64 x 64 tile of launch_gemm_splitk (same units and slices).
// T: bf16_t or fp16_t -- both are 2-byte elements on the same MFMA lane map (Mfma<T> / H16<T>), so the ring, its flags and the staging are one code.
template <typename T, int EPI, int BM, int BN, int CWM, int CWN, int NL, int SLOTS, bool SPLIT, int WAUX>
__global__ __launch_bounds__(64 * (CWM * CWN + NL)) void gemm_ring_kernel(GemmArgs<T, T> p) {
    using TI = T;
    using TO = T;
    static_assert(sizeof(T) == 2, "the ring moves 128-byte K-rows of 16-bit elements");
    constexpr int NC = CWM * CWN;                               // consumer waves: 0 .. NC-1; loader waves: NC .. NC+NL-1
    constexpr int WTM = BM / CWM, WTN = BN / CWN, FM = WTM / 32, FN = WTN / 32;
    constexpr int XG = BM / 8, G = (BM + BN) / 8, GPW = G / NL;     // 8-row groups of a slot (X first), groups per loader wave
    constexpr int SLOT = (BM + BN) * 128;
    constexpr int FLAGS = SLOTS * SLOT;                         // FULL[SLOTS][NL] then FREE[SLOTS][NC], u32
    constexpr unsigned SPIN_LIMIT = 1u << 20;                   // ~40 ms of polling before a wave gives up
    static_assert(FM >= 1 && FN >= 1 && WTM % 32 == 0 && WTN % 32 == 0 && G % NL == 0, "ring tile");
    static_assert(SLOTS >= 5 && 2 * GPW <= 63, "ring depth / vmcnt range");
    static_assert(!(EPI == EPI_SWIGLU) || !SPLIT, "gated epilogue on full-K tiles only");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    typedef const __attribute__((address_space(1))) void* gptr_t;
    typedef __attribute__((address_space(3))) void* lptr_t;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // workgroup -> (row block, column block, slice): the split-K mapping of gemm_nt_kernel (the row blocks of one (W tile, slice) pair take
    // consecutive places in one XCD's queue), with one slice for the full-K tiles
    const int tiles_n = (p.N + BN - 1) / BN, tiles_m = (p.M + BM - 1) / BM, S = SPLIT ? p.splitk : 1;
    const int x8 = (int)blockIdx.x & 7, j8 = (int)blockIdx.x >> 3;
    const int pair = (j8 / tiles_m) * 8 + x8;
    if (pair >= tiles_n * S) return;
    const int tile_m = j8 % tiles_m, tile_n = pair / S, ks = pair % S;
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const int nk_all = p.K / Ty<TI>::KE;
    const int kt_begin = SPLIT ? (int)((long)ks * nk_all / p.splitk) : 0;
    const int kt_end = SPLIT ? (int)((long)(ks + 1) * nk_all / p.splitk) : nk_all;
    const int nk = kt_end - kt_begin;

    const unsigned lds0 = (unsigned)(size_t)(lptr_t)smem;
    const unsigned full_w = lds0 + FLAGS, free_w = full_w + SLOTS * NL * 4;
    if (tid < SLOTS * (NL + NC)) reinterpret_cast<unsigned*>(smem + FLAGS)[tid] = 0u;
    __syncthreads();

    // Wait until every word of [base, base + 4 * n) is >= target. Lane l polls word l % n; one ds_read + its wait per poll, in one asm
    // statement (the result is ready when the statement ends).
    bool broken = false;
    auto wait_words = [&](unsigned base, int n, unsigned target) {
        const unsigned addr = base + (unsigned)(lane % n) * 4u;
        for (unsigned spin = 0; !broken; ++spin) {
            unsigned v;
            asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(addr) : "memory");
            if (__builtin_amdgcn_ballot_w64(v < target) == 0) break;
            if (spin >= SPIN_LIMIT) {
                broken = true;
                if (lane == 0) atomicOr(&ring_error_word, 1u);
                break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
    };
    auto post_word = [&](unsigned addr, unsigned v) { asm volatile("ds_write_b32 %0, %1" ::"v"(addr), "v"(v) : "memory"); };

    f32x16 acc[FN][FM];
    if (wave >= NC) {
        // ---- loader wave lw: groups lw * GPW .. lw * GPW + GPW - 1 of every slot. Lane l fills physical chunk (l & 7) of row (l >> 3) of
        // the group, i.e. fetches logical chunk (l & 7) ^ ((row >> 1) & 7) of that row (rows clamped into the matrix).
        const int lw = wave - NC;
        const unsigned char* src[GPW];
#pragma unroll
        for (int i = 0; i < GPW; ++i) {
            const int g = lw * GPW + i;
            const int lr = (g < XG ? g : g - XG) * 8 + (lane >> 3), c = (lane & 7) ^ ((lr >> 1) & 7);
            const unsigned char* base = g < XG ? reinterpret_cast<const unsigned char*>(p.X + (long)min(m0 + lr, p.M - 1) * p.ldx)
                                               : reinterpret_cast<const unsigned char*>(p.W + (long)min(n0 + lr, p.N - 1) * p.ldw);
            src[i] = base + c * 16 + (long)kt_begin * 128;
        }
        const unsigned my_full = full_w + lw * 4;
        int slot = 0, lap = 0;                                  // slot of K-tile kt and kt / SLOTS
        for (int kt = 0; kt < nk; ++kt) {
            if (kt >= SLOTS) wait_words(free_w + slot * NC * 4, NC, (unsigned)lap);     // every consumer is done with K-tile kt - SLOTS
            const long koff = (long)kt * 128;
#pragma unroll
            for (int i = 0; i < GPW; ++i) {
                const int g = lw * GPW + i;                     // wave-uniform: X rows at the default policy, W rows at WAUX
                unsigned char* dst = smem + slot * SLOT + g * 1024;
                if (WAUX == 0 || g < XG) __builtin_amdgcn_global_load_lds((gptr_t)(src[i] + koff), (lptr_t)dst, 16, 0, 0);
                else __builtin_amdgcn_global_load_lds((gptr_t)(src[i] + koff), (lptr_t)dst, 16, 0, WAUX);
            }
            if (kt >= 2) {                                      // K-tile kt - 2 has landed: publish it, kt - 1 and kt stay in flight
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * GPW) : "memory");
                const int ps = slot >= 2 ? slot - 2 : slot + SLOTS - 2;
                post_word(my_full + ps * NL * 4, (unsigned)((kt - 2) / SLOTS + 1));
            }
            if (++slot == SLOTS) { slot = 0; ++lap; }
        }
        // the last two K-tiles
        if (nk >= 2) {
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(GPW) : "memory");
            const int kt = nk - 2;
            post_word(my_full + (kt % SLOTS) * NL * 4, (unsigned)(kt / SLOTS + 1));
        }
        if (nk >= 1) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const int kt = nk - 1;
            post_word(my_full + (kt % SLOTS) * NL * 4, (unsigned)(kt / SLOTS + 1));
        }
    } else {
        // ---- consumer wave (cm, cn): WTM x WTN of the tile, fragments as in gemm_nt_kernel's SA_FRAGS
        const int cm = wave / CWN, cn = wave % CWN;
        const int frow = lane & 31, fch = lane >> 5;
#pragma unroll
        for (int j = 0; j < FN; ++j)
#pragma unroll
            for (int i = 0; i < FM; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[j][i][r] = 0.f;
        int xo[FM], wo[FN];                                     // fragment row offsets; the chunk of step kk is ((kk * 2 + fch) ^ swz) << 4
        int xs[FM], ws[FN];
#pragma unroll
        for (int i = 0; i < FM; ++i) {
            const int row = cm * WTM + i * 32 + frow;
            xo[i] = row * 128; xs[i] = (row >> 1) & 7;
        }
#pragma unroll
        for (int j = 0; j < FN; ++j) {
            const int row = cn * WTN + j * 32 + frow;
            wo[j] = BM * 128 + row * 128; ws[j] = (row >> 1) & 7;
        }
        const unsigned my_free = free_w + wave * 4;
        int slot = 0, lap = 0;
        for (int kt = 0; kt < nk; ++kt) {
            wait_words(full_w + slot * NL * 4, NL, (unsigned)(lap + 1));
            asm volatile("" ::: "memory");
            const unsigned char* cur = smem + slot * SLOT;
            u32x4 xf[4][FM], wf[4][FN];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
#pragma unroll
                for (int i = 0; i < FM; ++i) xf[kk][i] = *reinterpret_cast<const u32x4*>(cur + xo[i] + (((kk * 2 + fch) ^ xs[i]) << 4));
#pragma unroll
                for (int j = 0; j < FN; ++j) wf[kk][j] = *reinterpret_cast<const u32x4*>(cur + wo[j] + (((kk * 2 + fch) ^ ws[j]) << 4));
            }
            // every fragment is in registers: hand the slot back, then multiply
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            post_word(my_free + slot * NC * 4, (unsigned)(lap + 1));
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                for (int j = 0; j < FN; ++j)
#pragma unroll
                    for (int i = 0; i < FM; ++i) Mfma<TI>::run(acc[j][i], wf[kk][j], xf[kk][i]);
            if (++slot == SLOTS) { slot = 0; ++lap; }
        }
    }
    __syncthreads();                                            // the ring is idle (loaders drained): its LDS stages the output tile

    // ---- epilogue: the tile through LDS (row pitch padded by 16 bytes), then whole 16-byte chunks of contiguous rows
    constexpr bool GLU = (EPI == EPI_SWIGLU);
    constexpr int OW = GLU ? BN / 2 : BN;
    constexpr int ES = SPLIT ? 4 : 2;                           // staged element bytes: fp32 slabs or T
    constexpr int ROWB = OW * ES, PITCH = ROWB + 16, CPR = ROWB / 16, EPC = 16 / ES;
    static_assert(ROWB % 16 == 0 && BM * PITCH <= SLOTS * SLOT, "output staging");
    if (wave < NC) {
        const int cm = wave / CWN, cn = wave % CWN;
#pragma unroll
        for (int i = 0; i < FM; ++i) {
            const int row = cm * WTM + i * 32 + (lane & 31);
#pragma unroll
            for (int j = 0; j < FN; ++j)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int ncol = cn * WTN + j * 32 + g * 8 + (lane >> 5) * 4;
                    const float v0 = acc[j][i][4 * g], v1 = acc[j][i][4 * g + 1], v2 = acc[j][i][4 * g + 2], v3 = acc[j][i][4 * g + 3];
                    if constexpr (GLU) {
                        // weight rows interleaved (gate_j, up_j): columns ncol..+3 = g0,u0,g1,u1 -> outputs ncol/2, ncol/2+1
                        store2(reinterpret_cast<TO*>(smem + row * PITCH + (ncol >> 1) * ES), silu_epi<TI>(v0) * v1, silu_epi<TI>(v2) * v3);
                    } else if constexpr (SPLIT) {
                        store4(reinterpret_cast<float*>(smem + row * PITCH + ncol * ES), v0, v1, v2, v3);
                    } else {
                        store4(reinterpret_cast<TO*>(smem + row * PITCH + ncol * ES), v0, v1, v2, v3);
                    }
                }
        }
    }
    __syncthreads();
    constexpr int NT = 64 * (NC + NL);
    const int n_out = GLU ? p.N / 2 : p.N, n0_out = GLU ? n0 / 2 : n0;
    for (int id = tid; id < BM * CPR; id += NT) {
        const int row = id / CPR, c = id % CPR;
        const int m = m0 + row, n = n0_out + c * EPC;
        if (m >= p.M || n >= n_out) continue;
        const u32x4 raw = *reinterpret_cast<const u32x4*>(smem + row * PITCH + c * 16);
        if constexpr (SPLIT) *reinterpret_cast<u32x4*>(p.part + ((long)ks * p.M + m) * p.N + n) = raw;
        else *reinterpret_cast<u32x4*>(p.C + (long)m * p.ldc + n) = raw;
    }
}

template <typename T, int EPI, int BM, int BN, int CWM, int CWN, int NL, int SLOTS, bool SPLIT, int WAUX>
static inline int launch_gemm_ring(const GemmArgs<T, T>& a, hipStream_t s) {
    const int S = SPLIT ? a.splitk : 1;
    const int grid = cdiv(cdiv(a.N, BN) * S, 8) * 8 * cdiv(a.M, BM);
    constexpr int NT = 64 * (CWM * CWN + NL);
    constexpr size_t lds = (size_t)SLOTS * (BM + BN) * 128 + (size_t)SLOTS * (NL + CWM * CWN) * 4;
    static_assert(lds <= 160 * 1024 && SLOTS * (NL + CWM * CWN) <= NT, "ring LDS / flag clear");
    a.bn_used = BN;
    auto kern = gemm_ring_kernel<T, EPI, BM, BN, CWM, CWN, NL, SLOTS, SPLIT, WAUX>;
    static AttrOnce attr;
    attr.ensure(kern, lds);
    GemmProfiler& pf = gemm_profiler();
    const bool prof = pf.enabled && pf.n < GemmProfiler::POOL;
    if (prof) (void)hipEventRecord(pf.ev[2 * pf.n], s);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(NT), lds, s, a);
    if (prof) {
        (void)hipEventRecord(pf.ev[2 * pf.n + 1], s);
        pf.cfg_of[pf.n] = gemm_cfg_id(BM, BN);
        pf.flops_of[pf.n] = 2.0 * a.M * a.N * a.K;
        const double outn = EPI == EPI_SWIGLU ? a.N / 2 : a.N;
        pf.bytes_of[pf.n] = ((double)a.M * a.K + (double)a.N * a.K) * 2.0 + (double)a.M * outn * 2.0;
        pf.slab_of[pf.n] = SPLIT ? (double)a.splitk * a.M * a.N * 4.0 : 0.0;
        ++pf.n;
    }
    return (int)hipGetLastError();
}

// Ring launch policy (Tuning::dring; 0 = off, 1 = on, 2 = on with non-temporal weight loads, +4 = any M <= 256 for tests).
// Returns -1 when the shape stays on the tiles of gemm_nt_kernel.
static inline int ring_mode(int M) {
    const int d = tuning().dring;
    if (!(d & 3) || M <= 0 || M > 256) return 0;
    if (M <= 128 && !(d & 4)) return 0;
    return d & 3;
}
template <typename T>
static inline int launch_gateup_ring(const GemmArgs<T, T>& a, hipStream_t s) {
    const int mode = ring_mode(a.M);
    if (!mode || a.bias || a.N % 8 != 0) return -1;
    if (mode == 2) return launch_gemm_ring<T, EPI_SWIGLU, 64, 160, 1, 5, 4, 5, false, 2>(a, s);
    return launch_gemm_ring<T, EPI_SWIGLU, 64, 160, 1, 5, 4, 5, false, 0>(a, s);
}
// split-K: the 64 x 64 units and slice count of launch_gemm_splitk, for slices of at least dring_min_kt K-tiles (default 0: never)
template <typename T>
static inline int launch_splitk_ring(const GemmArgs<T, T>& a, hipStream_t s) {
    const int mode = ring_mode(a.M);
    const int min_kt = tuning().dring_min_kt;
    if (!mode || min_kt <= 0 || (a.K / Ty<T>::KE) / a.splitk < min_kt) return -1;
    if (mode == 2) return launch_gemm_ring<T, EPI_BIAS, 64, 64, 2, 2, 4, 8, true, 2>(a, s);
    return launch_gemm_ring<T, EPI_BIAS, 64, 64, 2, 2, 4, 8, true, 0>(a, s);
}

// Host check of the ring's give-up word (synchronous): 0 = every wait was satisfied since the last reset.
static inline int ring_error(bool reset) {
    unsigned v = 0;
    if (hipMemcpyFromSymbol(&v, HIP_SYMBOL(ring_error_word), sizeof(v)) != hipSuccess) return SA_ERR_STATE;
    if (reset && v) {
        const unsigned z = 0;
        (void)hipMemcpyToSymbol(HIP_SYMBOL(ring_error_word), &z, sizeof(z));
    }
    return v ? SA_ERR_STATE : SA_OK;
}

}  // namespace sa
