// What the two ranking files share (rank.hip: one table; rank_mixed.hip: the queries of one call ranked against different
// tables): the score, the pre-pass's sum of squares, the tile core's operand loader, the insertion into a query's
// candidate list and the merge of a query's strip lists. One definition each, so that a (query, row) pair has the same
// bits and a list the same order whichever file's kernels formed them.
#pragma once
#include <math.h>

#include "gemm_core.h"

#define RANK_MAX_K 128          // candidate lists: 64 queries x k x 8 B of LDS next to the tile core's 36 KB
#define RANK_SMALL_K 16
#define RANK_MID_K 64           // 70 KB of LDS in all: still two workgroups per CU (128: 100 KB, one)
#define RANK_MAX_STRIPS 64      // one lane of the merging wave per strip
#define RANK_TILE_LD 65         // score tile [64][65] (reuses the tile core's LDS)

__device__ __forceinline__ float rank_score(float dot, float rinv, float qinv) {
    const float s = (dot * rinv) * qinv;
    return s == s ? s : -INFINITY;          // (a NaN has no place in a total order: it ranks last)
}

// |v|^2 of one row by one wave (every lane gets the sum); score kind 1 (the plain dot) reads nothing and gives 0.
__device__ __forceinline__ float rank_sumsq(const float *__restrict__ v, int D, int lane, int score_kind) {
    float ss = 0.f;
    if (score_kind == 0)
        for (int c = lane; c < D; c += 64) ss += v[c] * v[c];
    return wave_sum(ss);
}
// The two per-row factors of rank_score from a row's norm.
__device__ __forceinline__ float rank_query_inv(float nrm, float eps, int score_kind) {
    return score_kind ? 1.f : 1.f / fmaxf(nrm, eps);      // (dot: (dot * 1) * 1 is the dot's own bits; eps is not read)
}
__device__ __forceinline__ float rank_row_inv(float nrm, int score_kind) {
    return score_kind ? 1.f : (nrm > 0.f ? 1.f / nrm : 0.f);      // (a zero row has no direction: it scores 0)
}

// ---------------------------------------------------------------------------------------------- operands
// Both operands are R-type (contiguous along k): A rows are query embeddings, B rows are table rows. The caller hands in
// this thread's two row pointers per operand; a row outside the operand is !ok (LD_FAST: a clamped valid row instead).
template <int MODE>
struct RankLoader {
    const float *pa0, *pa1, *pb0, *pb1, *sa, *sb;
    bool a0, a1, b0, b1;
    int c, K, left;

    __device__ __forceinline__ void init(const float *a_safe, const float *b_safe, int K_) {
        sa = a_safe;
        sb = b_safe;
        K = K_;
        c = stage_col(false);
        left = (K + GT_BK - 1) / GT_BK;
    }
    __device__ __forceinline__ f32x4 a(int slot, bool &ok) {
        return ld4_pred<MODE>(sa, slot ? pa1 : pa0, c, K, slot ? a1 : a0, ok);
    }
    __device__ __forceinline__ f32x4 b(int slot, bool &ok) {
        return ld4_pred<MODE>(sb, slot ? pb1 : pb0, c, K, slot ? b1 : b0, ok);
    }
    __device__ __forceinline__ void next() {
        const bool go = left > 1;           // freeze on the last step (surplus pipeline loads)
        left -= go ? 1 : 0;
        c += go ? GT_BK : 0;
    }
};

// ---------------------------------------------------------------------------------------------- candidate lists
// (s, row) into the list S_ / R_ of `len` entries, sorted by falling score, that keeps the k best. Rows arrive in
// increasing order, so the newcomer goes behind every entry of its own score; a full list drops its last entry (the
// caller has checked that s beats it strictly). Returns the new length.
__device__ __forceinline__ int rank_list_insert(float *S_, int *R_, int len, int k, float s, int row) {
    int p = len < k ? len : k - 1;
    while (p > 0 && S_[p - 1] < s) {
        S_[p] = S_[p - 1];
        R_[p] = R_[p - 1];
        --p;
    }
    S_[p] = s;
    R_[p] = row;
    return len < k ? len + 1 : len;
}

// One wave merges one query's strip lists into out_rows / out_scores [k]: lane l holds the head of strip l's list, which
// starts at cand_s / cand_r [base] (base < 0: this lane has no list). Strips cover increasing rows, so on equal scores the
// lower lane is the smaller row. Every lane of the wave calls it (shuffles); `live` false writes nothing.
__device__ __forceinline__ void rank_merge_lists(bool live, int lane, long long base, int k,
                                                 const float *__restrict__ cand_s, const int *__restrict__ cand_r,
                                                 long long *__restrict__ out_rows, float *__restrict__ out_scores) {
    int pos = 0;
    float hs = -INFINITY;
    int hr = -1;
    if (base >= 0 && k > 0) {
        hs = cand_s[base];
        hr = cand_r[base];
    }
    for (int j = 0; j < k; ++j) {
        float bs = hs;
        int bv = hr >= 0 ? 1 : 0, bl = lane;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float os = __shfl_xor(bs, o, 64);
            const int ov = __shfl_xor(bv, o, 64), ol = __shfl_xor(bl, o, 64);
            const bool better = ov != bv ? ov > bv : (os != bs ? os > bs : ol < bl);
            if (better) {
                bs = os;
                bv = ov;
                bl = ol;
            }
        }
        if (lane == bl && live) {
            out_rows[j] = bv ? (long long)hr : -1;
            out_scores[j] = bv ? hs : -INFINITY;
            if (bv) {
                ++pos;
                const bool more = pos < k;
                hs = more ? cand_s[base + pos] : -INFINITY;
                hr = more ? cand_r[base + pos] : -1;
            }
        }
    }
}
