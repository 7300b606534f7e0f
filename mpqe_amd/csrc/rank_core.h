// What the two ranking files share (rank.hip: one table; rank_mixed.hip: the queries of one call ranked against different
// tables): the score, the pre-pass's sum of squares and query branch, the operand loader, the gathered pair tile, the list
// insertion, the strip walk (tile loop, threshold rule, barriers), the merge and the finishing wave, and on the host the
// strip rule and the dispatch on list capacity and load mode. One definition each, so that a (query, row) pair has the
// same bits and a list the same order whichever file's kernels formed them. The __global__ kernels stay in the two files:
// they declare their __shared__ arrays, leave ahead of any barrier where they must and fill in a record of what differs.
#pragma once
#include <math.h>

#include <type_traits>

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

// ---------------------------------------------------------------------------------------------- pre-pass, queries
// One wave per query row v = q[j]: its factor, "no target yet", counters zeroed. cntx: the one-table call's second counter,
// or the literal nullptr -- told apart by type, here and in rank_finish_wave, so that no kernel branches on the pointer
// (in the finishing wave that branch put the two counters' loads one behind the other).
template <class Cntx>
__device__ __forceinline__ void rank_prep_query(const float *__restrict__ v, int D, int lane, float eps, int score_kind,
                                                long long j, float *__restrict__ qinv, float *__restrict__ tsc,
                                                int *__restrict__ trow, int *__restrict__ cnt, Cntx cntx) {
    const float ss = rank_sumsq(v, D, lane, score_kind);
    if (lane != 0) return;
    qinv[j] = rank_query_inv(sqrtf(ss), eps, score_kind);
    tsc[j] = -INFINITY;
    trow[j] = -1;
    cnt[j] = 0;
    if constexpr (!std::is_same<Cntx, std::nullptr_t>::value) cntx[j] = 0;
}

// ---------------------------------------------------------------------------------------------- listed pairs
// Scores of up to 64 listed (query, row) pairs as the DIAGONAL of a tile whose A rows and B rows are both gathered, so a
// pair gets the bits the strip walk gives it. pair(j) names pair j of the workgroup: !listed = no such pair, listed and
// !ok = a pair whose row is outside the table (flagged). `mine`: this thread holds the dot of a good pair.
struct RankPair {
    bool listed, ok;
    long long qi, r;
};
struct RankPairDot {
    bool mine;
    long long qi, r;
    float dot;
};
template <int MODE, class PairOf>
__device__ __forceinline__ RankPairDot rank_pair_tile(const float *__restrict__ q, const float *__restrict__ table, int D,
                                                      const PairOf &pair, float *smem, int32_t *err) {
    RankLoader<MODE> L;
    L.init(q, table, D);
    {
        RankPair p = pair(stage_row(false, 0));
        L.a0 = L.b0 = p.ok;
        L.pa0 = q + (p.ok ? p.qi : 0) * D;
        L.pb0 = table + (p.ok ? p.r : 0) * D;
        p = pair(stage_row(false, 1));
        L.a1 = L.b1 = p.ok;
        L.pa1 = q + (p.ok ? p.qi : 0) * D;
        L.pb1 = table + (p.ok ? p.r : 0) * D;
    }
    f32x16 acc;
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[g] = 0.f;
    gemm_block<false, false>(acc, L, L.left, smem);

    const int col = acc_col();
    RankPairDot out = {false, 0, 0, 0.f};
#pragma unroll
    for (int g = 0; g < 16; ++g)
        if (acc_row(g) == col) {
            out.dot = acc[g];
            out.mine = true;
        }
    if (!out.mine) return out;
    const RankPair p = pair(col);
    out.qi = p.qi;
    out.r = p.r;
    out.mine = p.listed && p.ok;
    if (p.listed && !p.ok) flag_error(err, MPQE_FLAG_BAD_INDEX);        // (the pre-pass left "no target" for the query)
    return out;
}

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

// ---------------------------------------------------------------------------------------------- the strip walk
// What a workgroup of either tile kernel walks: `live` queries (block rows 0 .. live - 1) against tiles
// [strip * tiles_per_strip, ...) of one table. Values only: a kernel fills the record in from its arguments or from its
// set record, derives a view that adds what differs, and hands it over by value. A view supplies
//   query(j)        the query of block row j (j < live)
//   bind(ok, sq)    this thread's share of the scan row's eligibility state (ok false: a dead row)
//   out_mask(cq)    bit j set = column cq + j is not eligible; taken before the count (cq a multiple of 16)
//   excluded(col)   a column that passed the threshold is not eligible after all; asked at insertion time
// The strip lists of block row j go to ((first + j) * S + strip) * k.
struct RankStrip {
    const float *q, *table, *rinv, *qinv, *tsc;         // rinv: the table's own rows' factors
    const int *trow;
    int *cnt, *cand_r;
    float *cand_s;
    long long N, first;
    int D, k, live, S, tiles_per_strip, strip;
};

// A workgroup meets its rows in increasing order, so of two equal scores the one already in a list is the smaller row
// and stays ahead: a newcomer must beat the k-th entry strictly. smem: the tile core's GT_SMEM_FLOATS, ls / lr: the
// lists [GT_BM][KL], llen [GT_BM] -- the kernel's own __shared__ arrays.
template <int MODE, int KL, class View>
__device__ __forceinline__ void rank_strip_walk(View V, float *smem, float *ls, int *lr, int *llen) {
    const int t = threadIdx.x;
    const int k = V.k;
    const long long N = V.N;
    if (t < GT_BM) llen[t] = 0;

    // the scan's view: 4 threads per query, 16 columns of the tile each
    const int srow = t >> 2, quarter = t & 3;
    const bool svalid = srow < V.live;
    const long long sq = svalid ? V.query(srow) : 0;
    const int tr = svalid ? V.trow[sq] : -1;
    const float ts = svalid ? V.tsc[sq] : 0.f;
    V.bind(svalid, sq);
    // the epilogue's view: one column, 16 query rows
    float qv[16];
#pragma unroll
    for (int g = 0; g < 16; ++g) {
        const int row = acc_row(g);
        qv[g] = row < V.live ? V.qinv[V.query(row)] : 0.f;
    }
    // (a row past the block: the block's first query, always there; its result is not used)
    const int a0 = stage_row(false, 0), a1 = stage_row(false, 1);
    const long long ar0 = V.query(a0 < V.live ? a0 : 0), ar1 = V.query(a1 < V.live ? a1 : 0);
    int count = 0;
    __syncthreads();

    for (int tile = 0; tile < V.tiles_per_strip; ++tile) {
        const long long c0 = ((long long)V.strip * V.tiles_per_strip + tile) * GT_BN;
        if (c0 >= N) break;
        RankLoader<MODE> L;
        L.init(V.q, V.table, V.D);
        const long long br0 = c0 + stage_row(false, 0), br1 = c0 + stage_row(false, 1);
        L.a0 = a0 < V.live;
        L.a1 = a1 < V.live;
        L.b0 = br0 < N;
        L.b1 = br1 < N;
        L.pa0 = V.q + ar0 * V.D;
        L.pa1 = V.q + ar1 * V.D;
        L.pb0 = V.table + (L.b0 ? br0 : N - 1) * V.D;
        L.pb1 = V.table + (L.b1 ? br1 : N - 1) * V.D;
        f32x16 acc;
#pragma unroll
        for (int g = 0; g < 16; ++g) acc[g] = 0.f;
        gemm_block<false, false>(acc, L, L.left, smem);         // (ends on a barrier: the LDS images are free)

        {
            const long long col = c0 + acc_col();
            const float rv = col < N ? V.rinv[col] : 0.f;
#pragma unroll
            for (int g = 0; g < 16; ++g) smem[acc_row(g) * RANK_TILE_LD + acc_col()] = rank_score(acc[g], rv, qv[g]);
        }
        __syncthreads();

        const unsigned out = V.out_mask(c0 + quarter * 16);
        unsigned pass = 0;
        float sc[16];
        {
            const int len = llen[srow];
            const bool full = len >= k;
            const float thr = full && k > 0 ? ls[srow * KL + k - 1] : 0.f;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const long long col = c0 + quarter * 16 + j;
                const float s = smem[srow * RANK_TILE_LD + quarter * 16 + j];
                sc[j] = s;
                const bool in = svalid && col < N && !(out & (1u << j));
                if (in && tr >= 0 && col != tr && (s > ts || (s == ts && col < tr))) ++count;
                if (in && k > 0 && (!full || s > thr)) pass |= 1u << j;
            }
        }
        if (k > 0) {
            for (int turn = 0; turn < 4; ++turn) {
                if (turn == quarter && pass) {
                    float *S_ = ls + srow * KL;
                    int *R_ = lr + srow * KL;
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        if (!(pass & (1u << j))) continue;
                        const float s = sc[j];
                        const int len = llen[srow];
                        if (len >= k && !(s > S_[k - 1])) continue;
                        const long long col = c0 + quarter * 16 + j;
                        if (V.excluded(col)) continue;
                        llen[srow] = rank_list_insert(S_, R_, len, k, s, (int)col);
                    }
                }
                __syncthreads();
            }
        } else {
            __syncthreads();        // (the next tile's operands overwrite the score tile)
        }
    }

    count += __shfl_xor(count, 1, 64);
    count += __shfl_xor(count, 2, 64);
    if (quarter == 0 && svalid && tr >= 0 && count) atomicAdd(&V.cnt[sq], count);
    for (int idx = t; idx < GT_BM * k; idx += 256) {
        const int row = idx / k, j = idx % k;
        if (row >= V.live) break;
        const bool have = j < llen[row];
        const long long dst = ((V.first + row) * V.S + V.strip) * k + j;
        V.cand_s[dst] = have ? ls[row * KL + j] : -INFINITY;
        V.cand_r[dst] = have ? lr[row * KL + j] : -1;
    }
}

// ---------------------------------------------------------------------------------------------- finish
// One wave writes query i's rank and target score and merges its strip lists (lane l: the list at `base`, < 0: none).
// good false: a query without a set -- no list, no target. cntx: the count to take out of the rank, or nullptr.
template <class Cntx>
__device__ __forceinline__ void rank_finish_wave(bool live, bool good, long long i, int lane, long long base, int k,
                                                 const float *__restrict__ cand_s, const int *__restrict__ cand_r,
                                                 const float *__restrict__ tsc, const int *__restrict__ trow,
                                                 const int *__restrict__ cnt, Cntx cntx,
                                                 long long *__restrict__ topk_rows, float *__restrict__ topk_scores,
                                                 long long *__restrict__ rank, float *__restrict__ target_scores) {
    if (live && lane == 0) {
        const int tr = good ? trow[i] : -1;
        long long less = 0;
        if constexpr (!std::is_same<Cntx, std::nullptr_t>::value) less = cntx[i];
        if (rank) rank[i] = tr >= 0 ? 1 + (long long)cnt[i] - less : -1;
        if (target_scores) target_scores[i] = tr >= 0 ? tsc[i] : NAN;
    }
    rank_merge_lists(live, lane, base, k, cand_s, cand_r, topk_rows + i * k, topk_scores + i * k);
}

// ---------------------------------------------------------------------------------------------- host
// The strip count of a call with `blocks` query blocks (or a bound on them) over `tiles` column tiles: enough workgroups
// to fill the device about three times over, a strip never empty, at most one strip per merging lane.
static inline void rank_strip_rule(long long blocks, long long tiles, int &S, int &tiles_per_strip) {
    long long want = (768 + blocks - 1) / blocks;
    if (want > RANK_MAX_STRIPS) want = RANK_MAX_STRIPS;
    if (want > tiles) want = tiles;
    if (want < 1) want = 1;
    const long long tps = (tiles + want - 1) / want;
    tiles_per_strip = (int)tps;
    S = (int)((tiles + tps - 1) / tps);
}

// f(std::integral_constant<int, KL>): the list capacity that holds k; g(... <int, MODE>): the operands' load mode.
template <class F>
static inline void rank_for_capacity(int k, F f) {
    if (k <= RANK_SMALL_K)
        f(std::integral_constant<int, RANK_SMALL_K>());
    else if (k <= RANK_MID_K)
        f(std::integral_constant<int, RANK_MID_K>());
    else
        f(std::integral_constant<int, RANK_MAX_K>());
}
template <class F>
static inline void rank_for_load_mode(bool vec, int64_t dim, F f) {
    if (vec && dim % GT_BK == 0)
        f(std::integral_constant<int, LD_FAST>());
    else if (vec)
        f(std::integral_constant<int, LD_PRED>());
    else
        f(std::integral_constant<int, LD_SCALAR>());
}
