// Shared helpers for the gfx950 kernels. Wavefront = 64 lanes everywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/mpqe_amd.h"

#define MPQE_WAVE 64

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

static inline int mpqe_launch_status() {
    return hipGetLastError() == hipSuccess ? MPQE_OK : MPQE_ERR_LAUNCH;
}

static inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Diagnostics switches (debug.hip): the value set by mpqe_debug_option(name, ...), `unset` otherwise. The library
// never reads the environment.
int mpqe_dbg_value(const char *name, int unset);
static inline bool dbg_on(const char *name) { return mpqe_dbg_value(name, 0) != 0; }
int mpqe_dbg_generation();       // bumped by every mpqe_debug_option call (plan caches key on it)

// Host-side copy of the template tables (reference data_utils.py:325-362).
struct TemplateDesc {
    int A, V, N, E, diam;
    int src[3], dst[3], rel_label[3], var_node[4];
};

static const TemplateDesc kTemplates[MPQE_Q_COUNT] = {
    /* 1-chain       */ {1, 1, 2, 1, 1, {0, 0, 0}, {1, 0, 0}, {0, 0, 0}, {0, 0, 0, 0}},
    /* 2-chain       */ {1, 2, 3, 2, 2, {0, 2, 0}, {2, 1, 0}, {1, 0, 0}, {0, 2, 0, 0}},
    /* 3-chain       */ {1, 3, 4, 3, 3, {0, 3, 2}, {3, 2, 1}, {2, 1, 0}, {0, 2, 4, 0}},
    /* 2-inter       */ {2, 1, 3, 2, 1, {0, 1, 0}, {2, 2, 0}, {0, 1, 0}, {0, 0, 0, 0}},
    /* 3-inter       */ {3, 1, 4, 3, 1, {0, 1, 2}, {3, 3, 3}, {0, 1, 2}, {0, 0, 0, 0}},
    /* 3-inter_chain */ {2, 2, 4, 3, 2, {0, 1, 3}, {2, 3, 2}, {0, 2, 1}, {0, 3, 0, 0}},
    /* 3-chain_inter */ {2, 2, 4, 3, 2, {0, 1, 3}, {3, 3, 2}, {1, 2, 0}, {0, 2, 0, 0}},
};

__device__ __forceinline__ void flag_error(int32_t *err, int32_t bit) {
    if (err) atomicOr(err, bit);
}

// entity id -> row of its table through node_map (NULL: the identity map, ids are table rows); -1 and
// MPQE_FLAG_BAD_NODE_ID (err may be NULL: flagged elsewhere) for an id or a row out of range
__device__ __forceinline__ long long lookup_row(const long long *node_map, long long map_len, long long id,
                                                long long table_rows, int32_t *err) {
    if (!node_map) {
        if (id < 0 || id >= table_rows) {
            flag_error(err, MPQE_FLAG_BAD_NODE_ID);
            return -1;
        }
        return id;
    }
    if (id < 0 || id >= map_len) {
        flag_error(err, MPQE_FLAG_BAD_NODE_ID);
        return -1;
    }
    const long long row = node_map[id];
    if (row < 0 || row >= table_rows) {
        flag_error(err, MPQE_FLAG_BAD_NODE_ID);
        return -1;
    }
    return row;
}

// The library's counter-based random stream: splitmix64's finaliser over a counter (mpqe_sample_negatives in optim.hip, the
// KG samplers in kg_sample.hip). Stateless, restated with Python ints by oracle/ref_cpu.py and tests/kg_sample_oracle.py.
__host__ __device__ __forceinline__ unsigned long long mpqe_mix64(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull;            // splitmix64
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// A word handed between workgroups of ONE launch (they may sit on different XCDs, each with an L2 of its own): written
// through / read at agent scope, no L2 write-back. (The host emulator runs a launch's workgroups one after the other.)
template <typename T>
__device__ __forceinline__ void agent_store(T *p, T v) {
#ifdef MPQE_EMU
    *p = v;
#else
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}
template <typename T>
__device__ __forceinline__ T agent_load(const T *p) {
#ifdef MPQE_EMU
    return *p;
#else
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// L2 normalisation of one embedding row by one wave: dst = v / ||v||_2 (no eps, reference
// encoders.py:42-43). ONE definition shared by the per-op kernel and the fused step so that both
// paths round identically (a last-bit difference in x0 can flip a ReLU downstream).
__device__ __forceinline__ float row_norm_store(const float *__restrict__ v, float *__restrict__ o, int D,
                                                int lane, bool vec) {
    float ss = 0.f;
    if (vec) {
        for (int c = lane * 4; c < D; c += 256) {
            f32x4 q = *reinterpret_cast<const f32x4 *>(v + c);
            ss += q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
        }
    } else {
        for (int c = lane; c < D; c += 64) ss += v[c] * v[c];
    }
    ss = wave_sum(ss);
    const float nrm = sqrtf(ss);
    if (vec) {
        for (int c = lane * 4; c < D; c += 256) {
            f32x4 q = *reinterpret_cast<const f32x4 *>(v + c);
            q[0] /= nrm; q[1] /= nrm; q[2] /= nrm; q[3] /= nrm;
            *reinterpret_cast<f32x4 *>(o + c) = q;
        }
    } else {
        for (int c = lane; c < D; c += 64) o[c] = v[c] / nrm;
    }
    return nrm;
}

// The same for a SUB-wave: `lpr` (a power of two <= 64) adjacent lanes own one row, so a wave
// normalises 64/lpr rows at once. Bit-identical to row_norm_store: there the lanes beyond D/4
// contribute exact zeros to the first butterfly steps, which is all that differs.
__device__ __forceinline__ int lanes_per_row(int D, bool vec) {
    if (!vec) return 64;
    int l = 1;
    while (l < 64 && l * 4 < D) l <<= 1;
    return l;
}
__device__ __forceinline__ void row_norm_store_sub(const float *__restrict__ v, float *__restrict__ o, int D,
                                                   int sub, int lpr, bool vec) {
    float ss = 0.f;
    if (vec) {
        for (int c = sub * 4; c < D; c += 4 * lpr) {
            f32x4 q = *reinterpret_cast<const f32x4 *>(v + c);
            ss += q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
        }
    } else {
        for (int c = sub; c < D; c += lpr) ss += v[c] * v[c];
    }
    for (int off = lpr >> 1; off > 0; off >>= 1) ss += __shfl_xor(ss, off, 64);
    const float nrm = sqrtf(ss);
    if (vec) {
        for (int c = sub * 4; c < D; c += 4 * lpr) {
            f32x4 q = *reinterpret_cast<const f32x4 *>(v + c);
            q[0] /= nrm; q[1] /= nrm; q[2] /= nrm; q[3] /= nrm;
            *reinterpret_cast<f32x4 *>(o + c) = q;
        }
    } else {
        for (int c = sub; c < D; c += lpr) o[c] = v[c] / nrm;
    }
}
