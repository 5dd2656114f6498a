// Boosted decoding: how a row's two greedy records -- A over the preferred set S (the masked lm_head partials), B over every column (the
// unmasked ones) -- become the token, the total and the plain reading of the boosted logits v'_i = v_i + beta * [i in S]. Shared by
// boost_head_kernel (boost.h) and a plain-C++ build used by the CPU tests (tests/native/boost_host.cpp). No launch or memory-model code.
// This is the single statement of the rules (surya_rec_set_boost, include/surya_amd.h).
//
// A record is (max, idx, sum) with sum = SUM_i exp(v_i - max) over its columns; idx is the first column that holds the max.
//   empty S      maxA = -inf (sumA = 0): the row is the unmasked row, whatever beta says; nothing is computed from A.
//   beta = +inf  "record A alone": token idxA, total sumA -- what the masked greedy head gives today. Rows that are not boosted carry it.
//   winner       a = fl32(maxA + beta), one fp32 addition; the token is idxA if a > maxB, idxB if a < maxB, the lower id on equality:
//                the first maximum of v' in fp32.
//   total        m = max(a, maxB); tot = sumB * exp(maxB - m) + sumA * (exp(a - m) - exp(maxA - m)). No exponent is positive, so no
//                beta overflows. 1 / tot is the winner's softmax probability under v'.
//   plain        plain_token = idxB; plain_prob = exp(v_tok - maxB) / sumB, v_tok = maxA or maxB according to the winner: the emitted
//                token's probability without the boost.
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

namespace sa {
namespace boost {

struct Out {
    int token; float tot; int plain_token; float plain_prob;
};

SA_HD Out combine(float maxA, int idxA, float sumA, float maxB, int idxB, float sumB, float beta) {
    Out o;
    o.plain_token = idxB;
    if (maxA == -INFINITY) {                                  // empty S: no (-inf) - (-inf) below
        o.token = idxB; o.tot = sumB; o.plain_prob = 1.0f / sumB;
        return o;
    }
    if (beta == INFINITY) {                                   // record A alone
        o.token = idxA; o.tot = sumA; o.plain_prob = expf(maxA - maxB) / sumB;
        return o;
    }
    const float a = maxA + beta;
    const bool winA = a > maxB || (a == maxB && idxA < idxB);
    const float m = a > maxB ? a : maxB;
    o.token = winA ? idxA : idxB;
    o.tot = sumB * expf(maxB - m) + sumA * (expf(a - m) - expf(maxA - m));
    o.plain_prob = expf((winA ? maxA : maxB) - maxB) / sumB;
    return o;
}

}  // namespace boost
}  // namespace sa
