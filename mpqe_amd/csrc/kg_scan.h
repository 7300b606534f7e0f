// The exclusive scan of one int per thread over a workgroup of 256 threads (4 waves), as mpqe_kg_rows places a word's rows
// (kg.hip) and the row samplers their chunk sums (kg_sample.hip): shuffles inside a wave, the waves' sums through LDS.
#pragma once
#include "common.h"

#define KG_SCAN_WAVES 4

// -> the sum of `v` over the threads below this one; `total`: over all of them. wsum: KG_SCAN_WAVES ints of the caller's LDS
// (declared in the kernel). Holds one barrier, so every thread of the workgroup calls it; the next call rewrites wsum, so
// the caller puts a barrier of its own between two calls.
__device__ __forceinline__ int kg_workgroup_scan(int v, int *wsum, int &total) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl(incl, lane >= o ? lane - o : lane, 64);
        if (lane >= o) incl += up;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < KG_SCAN_WAVES; ++i) {
        before += i < wave ? wsum[i] : 0;
        total += wsum[i];
    }
    return before + incl - v;
}
