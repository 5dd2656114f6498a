// Plain-C++ build of surya_amd/csrc/boost_core.h for tests/test_boost_cpu.py (g++ -ffp-contract=off): `n` rows of two records each.
#include "../../surya_amd/csrc/boost_core.h"

extern "C" void boost_combine_host(int n, const float* maxA, const int* idxA, const float* sumA, const float* maxB, const int* idxB,
                                   const float* sumB, const float* beta, int* token, float* tot, int* plain_token, float* plain_prob) {
    for (int i = 0; i < n; ++i) {
        const sa::boost::Out o = sa::boost::combine(maxA[i], idxA[i], sumA[i], maxB[i], idxB[i], sumB[i], beta[i]);
        token[i] = o.token; tot[i] = o.tot; plain_token[i] = o.plain_token; plain_prob[i] = o.plain_prob;
    }
}
