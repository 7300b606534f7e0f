// The two metrics of the reference's evaluation (utils.py:25-95) on scores that are already on the device. Integer work
// only: comparisons, counts, a sort of 32-bit keys and integer sums -- no float arithmetic, no float atomics, so a call
// gives the same bits every run.
//
// mpqe_eval_counts  _get_perc_scores (utils.py:25-32): per query the number of its negatives that score below / not above
//   its target, from the flat score vector forward() returns (B target scores, then the negatives' in CSR order). Two
//   launches over the same queries: a list of up to EV_LONG scores is one wave's (four queries a workgroup, a butterfly of
//   the two counts); a longer one -- the complement of an answer set, up to a whole mode -- is a workgroup's, in rounds of
//   EV_THREADS scores, combined through LDS with integer adds. Each kernel leaves the other's queries alone. The
//   comparisons are the hardware's IEEE ones: NaN is neither below nor equal, -0.0 equals +0.0.
//
// mpqe_eval_auc  the Mann-Whitney statistic behind ROC-AUC, doubled so that it is an integer:
//   U2 = sum over positives p of 2 |{negatives < p}| + |{negatives == p}|,   AUC = U2 / (2 n_pos n_neg).
//   Scores become order-preserving 32-bit keys (ev_key), the negatives' keys are sorted by the library's own radix sort
//   (radix_sort.h), every positive binary-searches its lower and upper bound (their sum is its term) and the workgroups'
//   sums are added to the output word with one 64-bit integer atomic each: integer adds commute, the result does not depend
//   on their order.
#include "radix_sort.h"

#define EV_THREADS 256
#define EV_WAVES 4
#define EV_LONG 512                 // lists longer than this are a workgroup's, not a wave's
#define EV_MAX_BLOCKS 1024          // mpqe_eval_auc: at most this many workgroups share the positives

// lo / hi of query q's list; false for a segment that is out of order or outside [0, total]
__device__ __forceinline__ bool ev_segment(const long long *__restrict__ off, long long q, long long total, long long *lo,
                                           long long *hi) {
    *lo = off[q];
    *hi = off[q + 1];
    return *lo >= 0 && *hi >= *lo && *hi <= total;
}

__global__ __launch_bounds__(EV_THREADS) void eval_counts_wave_kernel(const float *__restrict__ scores,
                                                                      const long long *__restrict__ off, long long B,
                                                                      long long total, long long *__restrict__ out,
                                                                      int32_t *err) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long q = (long long)blockIdx.x * EV_WAVES + wave;
    if (q >= B) return;                             // (wave-uniform, as is every exit below; no workgroup barrier here)
    long long lo, hi;
    if (!ev_segment(off, q, total, &lo, &hi)) {
        if (lane == 0) flag_error(err, MPQE_FLAG_BAD_INDEX);
        return;
    }
    if (hi - lo > EV_LONG) return;                  // eval_counts_block_kernel's
    const float t = scores[q];
    const float *neg = scores + B;
    int lt = 0, le = 0;
    for (long long j = lo + lane; j < hi; j += 64) {
        const float s = neg[j];
        lt += s < t ? 1 : 0;
        le += s <= t ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lt += __shfl_xor(lt, o, 64);
        le += __shfl_xor(le, o, 64);
    }
    if (lane == 0) {
        out[q] = lt;
        out[B + q] = le;
    }
}

__global__ __launch_bounds__(EV_THREADS) void eval_counts_block_kernel(const float *__restrict__ scores,
                                                                       const long long *__restrict__ off, long long B,
                                                                       long long total, long long *__restrict__ out) {
    __shared__ long long part[2][EV_WAVES];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long q = blockIdx.x;
    long long lo, hi;
    if (!ev_segment(off, q, total, &lo, &hi) || hi - lo <= EV_LONG) return;         // (uniform; the wave kernel flags / counts)
    const float tgt = scores[q];
    const float *neg = scores + B;
    int lt = 0, le = 0;                             // (total < 2^31: a lane's count fits, and so does a wave's)
    for (long long j = lo + t; j < hi; j += EV_THREADS) {
        const float s = neg[j];
        lt += s < tgt ? 1 : 0;
        le += s <= tgt ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lt += __shfl_xor(lt, o, 64);
        le += __shfl_xor(le, o, 64);
    }
    if (lane == 0) {
        part[0][wave] = lt;
        part[1][wave] = le;
    }
    __syncthreads();
    if (t < 2) {
        long long sum = 0;
#pragma unroll
        for (int w = 0; w < EV_WAVES; ++w) sum += part[t][w];
        out[(long long)t * B + q] = sum;
    }
}

extern "C" int mpqe_eval_counts(const float *scores, const int64_t *neg_offsets, int64_t B, int64_t total, int64_t *counts,
                                int32_t *err, void *stream) {
    if (B < 0 || total < 0) return MPQE_ERR_INVALID_ARG;
    if (B >= ((int64_t)1 << 31) || total >= ((int64_t)1 << 31)) return MPQE_ERR_UNSUPPORTED;
    if (B == 0) return MPQE_OK;
    if (!scores || !neg_offsets || !counts) return MPQE_ERR_INVALID_ARG;
    hipStream_t s = as_stream(stream);
    const long long *off = reinterpret_cast<const long long *>(neg_offsets);
    long long *out = reinterpret_cast<long long *>(counts);
    hipLaunchKernelGGL(eval_counts_wave_kernel, dim3((unsigned)((B + EV_WAVES - 1) / EV_WAVES)), dim3(EV_THREADS), 0, s,
                       scores, off, (long long)B, (long long)total, out, err);
    if (total > EV_LONG)                            // (no list can be that long otherwise)
        hipLaunchKernelGGL(eval_counts_block_kernel, dim3((unsigned)B), dim3(EV_THREADS), 0, s, scores, off, (long long)B,
                           (long long)total, out);
    return mpqe_launch_status();
}

// ----------------------------------------------------------------------------------------------------------- ROC-AUC
// A score as the host path ranks it (np.nan_to_num, then == on doubles): NaN is 0.0, -0.0 is +0.0; then the usual map of
// IEEE bits to unsigned keys of the same order (negative: all bits flipped, otherwise the sign bit set). +-inf stay the
// extremes and tie among themselves.
__device__ __forceinline__ unsigned ev_key(float s) {
    if (s != s) s = 0.f;
    unsigned b = __float_as_uint(s);
    if (b == 0x80000000u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__global__ __launch_bounds__(EV_THREADS) void eval_auc_keys_kernel(const float *__restrict__ neg, long long n,
                                                                   unsigned *__restrict__ keys) {
    const long long i = (long long)blockIdx.x * EV_THREADS + threadIdx.x;
    if (i < n) keys[i] = ev_key(neg[i]);
}

__global__ __launch_bounds__(EV_THREADS) void eval_auc_search_kernel(const float *__restrict__ pos, long long n_pos,
                                                                     const unsigned *__restrict__ keys, long long n_neg,
                                                                     unsigned long long *__restrict__ out) {
    __shared__ unsigned long long part[EV_THREADS];
    const int t = threadIdx.x;
    unsigned long long acc = 0ull;
    for (long long i = (long long)blockIdx.x * EV_THREADS + t; i < n_pos; i += (long long)gridDim.x * EV_THREADS) {
        const unsigned k = ev_key(pos[i]);
        long long a = 0, b = n_neg;                 // the first index whose key is >= k
        while (a < b) {
            const long long mid = (a + b) >> 1;
            if (keys[mid] < k) a = mid + 1; else b = mid;
        }
        const long long below = a;
        b = n_neg;                                  // the first index whose key is > k (not before `below`)
        while (a < b) {
            const long long mid = (a + b) >> 1;
            if (keys[mid] <= k) a = mid + 1; else b = mid;
        }
        acc += (unsigned long long)(below + a);     // 2 below + (a - below) ties
    }
    part[t] = acc;
    __syncthreads();
    for (int s = EV_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) part[t] += part[t + s];
        __syncthreads();
    }
    if (t == 0 && part[0]) atomicAdd(out, part[0]);
}

// workspace: keys [n_neg] | sorted keys [n_neg] | the sort's item numbers [n_neg] (unused) | the sort's scratch
static inline size_t ev_keys_bytes(int64_t n_neg) { return align_up((size_t)n_neg * 4, 256); }

extern "C" size_t mpqe_eval_auc_workspace_bytes(int64_t n_pos, int64_t n_neg) {
    if (n_pos < 1 || n_neg < 1 || n_pos >= ((int64_t)1 << 31) || n_neg >= ((int64_t)1 << 31)) return 0;
    return 3 * ev_keys_bytes(n_neg) + radix_sort_tmp_bytes<unsigned>((long long)n_neg);
}

extern "C" int mpqe_eval_auc(const float *pos, int64_t n_pos, const float *neg, int64_t n_neg, uint64_t *u2, void *workspace,
                             size_t workspace_bytes, void *stream) {
    if (n_pos < 1 || n_neg < 1 || !pos || !neg || !u2) return MPQE_ERR_INVALID_ARG;
    if (n_pos >= ((int64_t)1 << 31) || n_neg >= ((int64_t)1 << 31)) return MPQE_ERR_UNSUPPORTED;
    if (!workspace || ((uintptr_t)workspace & 3) || ((uintptr_t)u2 & 7)) return MPQE_ERR_INVALID_ARG;
    if (workspace_bytes < mpqe_eval_auc_workspace_bytes(n_pos, n_neg)) return MPQE_ERR_WORKSPACE;
    hipStream_t s = as_stream(stream);
    char *wb = reinterpret_cast<char *>(workspace);
    const size_t kb = ev_keys_bytes(n_neg);
    unsigned *keys = reinterpret_cast<unsigned *>(wb), *sorted = reinterpret_cast<unsigned *>(wb + kb);
    int *perm = reinterpret_cast<int *>(wb + 2 * kb);
    if (hipMemsetAsync(u2, 0, sizeof(uint64_t), s) != hipSuccess) return MPQE_ERR_LAUNCH;
    hipLaunchKernelGGL(eval_auc_keys_kernel, dim3((unsigned)((n_neg + EV_THREADS - 1) / EV_THREADS)), dim3(EV_THREADS), 0, s,
                       neg, (long long)n_neg, keys);
    const int st = radix_sort_pairs_own<unsigned>(wb + 3 * kb, (const unsigned *)keys, sorted, nullptr, perm,
                                                  (long long)n_neg, 32, s);
    if (st != MPQE_OK) return st;
    long long blocks = (n_pos + EV_THREADS - 1) / EV_THREADS;
    if (blocks > EV_MAX_BLOCKS) blocks = EV_MAX_BLOCKS;
    hipLaunchKernelGGL(eval_auc_search_kernel, dim3((unsigned)blocks), dim3(EV_THREADS), 0, s, pos, (long long)n_pos,
                       (const unsigned *)sorted, (long long)n_neg, reinterpret_cast<unsigned long long *>(u2));
    return mpqe_launch_status();
}

// ------------------------------------------------------------------------------------------- ROC-AUC of S segments at once
// mpqe_eval_auc_segments: u2[s] = mpqe_eval_auc's statistic of (pos[pos_off[s] .. pos_off[s + 1]), neg[neg_off[s] ..
// neg_off[s + 1])) for every s, in one call with no host read. A negative becomes the 64-bit key (segment << 32 | ev_key);
// one sort of those keys (radix_sort.h is templated on the key) leaves every segment where it was, its keys in order, so a
// positive searches its own segment's bounds only: an equal score on the other side of a boundary has another key and is
// outside them. The terms are added to u2[s] with 64-bit integer atomics; an empty side gives 0. A segment whose offsets
// are out of order or outside the arrays is left at 0.

// the segment of item i: the last s in [0, S) with off[s] <= i (empty segments have no items)
__device__ __forceinline__ long long ev_segment_of(const long long *__restrict__ off, long long S, long long i) {
    long long a = 0, b = S;
    while (b - a > 1) {
        const long long mid = (a + b) >> 1;
        if (off[mid] <= i) a = mid; else b = mid;
    }
    return a;
}

__global__ __launch_bounds__(EV_THREADS) void eval_seg_keys_kernel(const float *__restrict__ neg, long long n,
                                                                   const long long *__restrict__ neg_off, long long S,
                                                                   unsigned long long *__restrict__ keys) {
    const long long i = (long long)blockIdx.x * EV_THREADS + threadIdx.x;
    if (i < n) keys[i] = ((unsigned long long)ev_segment_of(neg_off, S, i) << 32) | ev_key(neg[i]);
}

__global__ __launch_bounds__(EV_THREADS) void eval_seg_search_kernel(const float *__restrict__ pos, long long n_pos,
                                                                     const long long *__restrict__ pos_off,
                                                                     const unsigned long long *__restrict__ keys,
                                                                     long long n_neg, const long long *__restrict__ neg_off,
                                                                     long long S, unsigned long long *__restrict__ out) {
    const long long i = (long long)blockIdx.x * EV_THREADS + threadIdx.x;
    if (i >= n_pos) return;
    const long long s = ev_segment_of(pos_off, S, i);
    long long plo, phi, lo, hi;
    if (!ev_segment(pos_off, s, n_pos, &plo, &phi) || i < plo || i >= phi) return;
    if (!ev_segment(neg_off, s, n_neg, &lo, &hi)) return;
    const unsigned long long k = ((unsigned long long)s << 32) | ev_key(pos[i]);
    long long a = lo, b = hi;                       // the first index of the segment whose key is >= k
    while (a < b) {
        const long long mid = (a + b) >> 1;
        if (keys[mid] < k) a = mid + 1; else b = mid;
    }
    const long long below = a;
    b = hi;                                         // the first whose key is > k
    while (a < b) {
        const long long mid = (a + b) >> 1;
        if (keys[mid] <= k) a = mid + 1; else b = mid;
    }
    const unsigned long long term = (unsigned long long)((below - lo) + (a - lo));
    if (term) atomicAdd(out + s, term);
}

// workspace: keys [n_neg] u64 | sorted keys [n_neg] u64 | the sort's item numbers [n_neg] (unused) | the sort's scratch
static inline size_t ev_seg_keys_bytes(int64_t n_neg) { return align_up((size_t)(n_neg > 0 ? n_neg : 1) * 8, 256); }

extern "C" size_t mpqe_eval_auc_segments_workspace_bytes(int64_t n_pos, int64_t n_neg, int64_t num_segments) {
    if (n_pos < 0 || n_neg < 0 || num_segments < 1) return 0;
    if (n_pos >= ((int64_t)1 << 31) || n_neg >= ((int64_t)1 << 31) || num_segments >= ((int64_t)1 << 31)) return 0;
    return 2 * ev_seg_keys_bytes(n_neg) + ev_keys_bytes(n_neg > 0 ? n_neg : 1) +
           radix_sort_tmp_bytes<unsigned long long>((long long)n_neg);
}

extern "C" int mpqe_eval_auc_segments(const float *pos, int64_t n_pos, const float *neg, int64_t n_neg,
                                      const int64_t *pos_off, const int64_t *neg_off, int64_t num_segments, uint64_t *u2,
                                      void *workspace, size_t workspace_bytes, void *stream) {
    if (n_pos < 0 || n_neg < 0 || num_segments < 1 || !pos_off || !neg_off || !u2) return MPQE_ERR_INVALID_ARG;
    if ((n_pos > 0 && !pos) || (n_neg > 0 && !neg)) return MPQE_ERR_INVALID_ARG;
    if (n_pos >= ((int64_t)1 << 31) || n_neg >= ((int64_t)1 << 31) || num_segments >= ((int64_t)1 << 31))
        return MPQE_ERR_UNSUPPORTED;
    if (!workspace || ((uintptr_t)workspace & 7) || ((uintptr_t)u2 & 7)) return MPQE_ERR_INVALID_ARG;
    if (workspace_bytes < mpqe_eval_auc_segments_workspace_bytes(n_pos, n_neg, num_segments)) return MPQE_ERR_WORKSPACE;
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(u2, 0, (size_t)num_segments * sizeof(uint64_t), s) != hipSuccess) return MPQE_ERR_LAUNCH;
    if (n_pos == 0 || n_neg == 0) return MPQE_OK;
    char *wb = reinterpret_cast<char *>(workspace);
    const size_t kb = ev_seg_keys_bytes(n_neg);
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(wb);
    unsigned long long *sorted = reinterpret_cast<unsigned long long *>(wb + kb);
    int *perm = reinterpret_cast<int *>(wb + 2 * kb);
    const long long *noff = reinterpret_cast<const long long *>(neg_off);
    hipLaunchKernelGGL(eval_seg_keys_kernel, dim3((unsigned)((n_neg + EV_THREADS - 1) / EV_THREADS)), dim3(EV_THREADS), 0, s,
                       neg, (long long)n_neg, noff, (long long)num_segments, keys);
    int seg_bits = 0;
    while (((int64_t)1 << seg_bits) < num_segments) ++seg_bits;
    const int st = radix_sort_pairs_own<unsigned long long>(wb + 2 * kb + ev_keys_bytes(n_neg), (const unsigned long long *)keys,
                                                            sorted, nullptr, perm, (long long)n_neg, 32 + seg_bits, s);
    if (st != MPQE_OK) return st;
    hipLaunchKernelGGL(eval_seg_search_kernel, dim3((unsigned)((n_pos + EV_THREADS - 1) / EV_THREADS)), dim3(EV_THREADS), 0, s,
                       pos, (long long)n_pos, reinterpret_cast<const long long *>(pos_off),
                       (const unsigned long long *)sorted, (long long)n_neg, noff, (long long)num_segments,
                       reinterpret_cast<unsigned long long *>(u2));
    return mpqe_launch_status();
}
