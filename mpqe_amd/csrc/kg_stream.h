// The keyed bijection of the KG samplers (include/mpqe_amd.h, "The random stream"): mpqe_kg_sample_rows draws its k-subsets
// with it (kg_sample.hip), mpqe_kg_sample_neighbours the sampled positions of a neighbour list (sage.hip). ONE definition, so
// that both draw from the same stream; tests/kg_sample_oracle.py restates it with Python ints.
#pragma once
#include "common.h"

#define KGS_FEISTEL_ROUNDS 8

// P(j) for the bijection of [0, c) keyed by `key`: Feistel rounds on two halves of h bits, (L, R) -> (R, L ^ F(round, R)),
// repeated until the value is below c (cycle walking: the orbit of a value below c returns below c).
__device__ __forceinline__ long long kgs_permute(unsigned long long key, long long c, int h, long long j) {
    const unsigned long long mask = (1ull << h) - 1ull;
    unsigned long long x = (unsigned long long)j;
    do {
        unsigned long long L = x >> h, R = x & mask;
#pragma unroll
        for (int r = 0; r < KGS_FEISTEL_ROUNDS; ++r) {
            const unsigned long long f = mpqe_mix64(key ^ (((unsigned long long)(r + 1) << 32) | R)) & mask;
            const unsigned long long nr = L ^ f;
            L = R;
            R = nr;
        }
        x = (L << h) | R;
    } while (x >= (unsigned long long)c);
    return (long long)x;
}
