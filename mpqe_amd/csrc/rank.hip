// Answering a query: Q query embeddings scored against EVERY row of one mode's entity table, with the rank of a target
// row and the k best rows per query, on the 64 x 64 fp32 MFMA tile core of gemm_core.h. The [Q, N] score matrix never
// reaches HBM: a workgroup owns 64 queries and a strip of consecutive 64-row column tiles, keeps the k best rows of each
// of its queries in LDS across the strip, and counts the rows that precede each query's target as it goes.
//
//   score(i, r) = ((q[i] . table[r]) * 1/|table[r]|) * 1/max(|q[i]|, eps)          (rank_score)
//
// The dot product is the tile core's fixed k-order MFMA chain and both factors are per-row values of a pre-pass, so a
// pair's score depends on q[i] and table[r] alone -- not on the tile, workgroup or launch that formed it. That is what
// lets four launches agree exactly:
//   rank_prep_kernel     1/|table[r]|, 1/max(|q[i]|, eps); counters zeroed
//   rank_pair_kernel     scores of listed (query, row) pairs as the diagonal of a tile whose A rows and B rows are both
//                        gathered: mode 0 the targets, mode 1 the exclusion lists (those that precede the target are
//                        counted, to be taken out of the rank)
//   rank_tile_kernel     all rows: counts against the target's score, per-strip candidate lists
//   rank_finish_kernel   merges a query's strip lists in strip order (one wave per query), writes rank and top-k
// Total order: higher fp32 score first, the smaller row on equal scores. Counters are integers (integer atomics: the sum
// does not depend on the order); no float atomics.
// rank_core.h holds what rank_mixed.hip (the queries of one call ranked against different tables) runs too: the score, the
// pre-pass's per-row factors, the operand loader, the list insertion and the merge.
#include "rank_core.h"

// ---------------------------------------------------------------------------------------------- pre-pass
__global__ __launch_bounds__(256) void rank_prep_kernel(const float *__restrict__ q, long long Q,
                                                        const float *__restrict__ table, long long N, int D, float eps,
                                                        int score_kind, float *__restrict__ rinv,
                                                        float *__restrict__ qinv,
                                                        float *__restrict__ tsc, int *__restrict__ trow,
                                                        int *__restrict__ cnt, int *__restrict__ cntx) {
    const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N + Q) return;
    const int lane = threadIdx.x & 63;
    const bool is_q = i >= N;
    const float *v = is_q ? q + (i - N) * D : table + i * D;
    const float ss = rank_sumsq(v, D, lane, score_kind);
    if (lane != 0) return;
    const float nrm = sqrtf(ss);
    if (is_q) {
        const long long j = i - N;
        qinv[j] = rank_query_inv(nrm, eps, score_kind);
        tsc[j] = -INFINITY;
        trow[j] = -1;
        cnt[j] = 0;
        cntx[j] = 0;
    } else {
        rinv[i] = rank_row_inv(nrm, score_kind);
    }
}

// ---------------------------------------------------------------------------------------------- listed pairs
// The query whose CSR segment holds entry e: the last i with off[i] <= e (bounded: a garbled offset array cannot send it
// outside [0, Q)); the caller checks e < off[i + 1].
__device__ __forceinline__ long long rank_entry_query(const long long *__restrict__ off, long long Q, long long e) {
    long long lo = 0, hi = Q - 1;
    while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        if (off[mid] <= e) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// mode 0: pair p = (p, target_rows[p]); mode 1: pair p = (query of entry p, excl_rows[p]). false: no such pair.
__device__ __forceinline__ bool rank_pair(int mode, long long p, long long Q, long long N,
                                          const long long *__restrict__ target_rows,
                                          const long long *__restrict__ off, const long long *__restrict__ excl,
                                          long long E, long long &qi, long long &r, bool &listed) {
    listed = false;
    qi = 0;
    r = 0;
    if (mode == 0) {
        if (p >= Q) return false;
        listed = true;
        qi = p;
        r = target_rows[p];
    } else {
        if (p >= E) return false;
        qi = rank_entry_query(off, Q, p);
        if (off[qi] > p || off[qi + 1] <= p) return false;
        listed = true;
        r = excl[p];
    }
    return r >= 0 && r < N;
}

template <int MODE>
__global__ __launch_bounds__(256) void rank_pair_kernel(int mode, const float *__restrict__ q, long long Q,
                                                        const float *__restrict__ table, long long N, int D,
                                                        const float *__restrict__ rinv, const float *__restrict__ qinv,
                                                        const long long *__restrict__ target_rows,
                                                        const long long *__restrict__ off,
                                                        const long long *__restrict__ excl, long long E,
                                                        float *__restrict__ tsc, int *__restrict__ trow,
                                                        int *__restrict__ cntx, int32_t *err) {
    __shared__ __attribute__((aligned(16))) float smem[GT_SMEM_FLOATS];
    const long long p0 = (long long)blockIdx.x * GT_BM;
    RankLoader<MODE> L;
    L.init(q, table, D);
    {
        long long qi, r;
        bool listed;
        bool ok = rank_pair(mode, p0 + stage_row(false, 0), Q, N, target_rows, off, excl, E, qi, r, listed);
        L.a0 = L.b0 = ok;
        L.pa0 = q + (ok ? qi : 0) * D;
        L.pb0 = table + (ok ? r : 0) * D;
        ok = rank_pair(mode, p0 + stage_row(false, 1), Q, N, target_rows, off, excl, E, qi, r, listed);
        L.a1 = L.b1 = ok;
        L.pa1 = q + (ok ? qi : 0) * D;
        L.pb1 = table + (ok ? r : 0) * D;
    }
    f32x16 acc;
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[g] = 0.f;
    gemm_block<false, false>(acc, L, L.left, smem);

    const int col = acc_col();
    float dot = 0.f;
    bool mine = false;
#pragma unroll
    for (int g = 0; g < 16; ++g)
        if (acc_row(g) == col) {
            dot = acc[g];
            mine = true;
        }
    if (!mine) return;
    const long long p = p0 + col;
    long long qi, r;
    bool listed;
    const bool ok = rank_pair(mode, p, Q, N, target_rows, off, excl, E, qi, r, listed);
    if (!listed) return;
    if (!ok) {
        flag_error(err, MPQE_FLAG_BAD_INDEX);       // (mode 0: the pre-pass left "no target" for this query)
        return;
    }
    const float s = rank_score(dot, rinv[r], qinv[qi]);
    if (mode == 0) {
        tsc[qi] = s;
        trow[qi] = (int)r;
        return;
    }
    if (p > off[qi] && p > 0) {           // lists are sorted: a repeated row counts once, a descent is the caller's error
        const long long prev = excl[p - 1];
        if (prev > r) flag_error(err, MPQE_FLAG_BAD_INDEX);
        if (prev == r) return;
    }
    const int tr = trow[qi];
    if (tr < 0 || r == tr) return;
    const float ts = tsc[qi];
    if (s > ts || (s == ts && r < tr)) atomicAdd(&cntx[qi], 1);
}

// ---------------------------------------------------------------------------------------------- all rows
// Is `row` in the sorted list excl[lo, hi)?
__device__ __forceinline__ bool rank_excluded(const long long *__restrict__ excl, long long lo, long long hi,
                                              long long row) {
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        const long long v = excl[mid];
        if (v == row) return true;
        if (v < row) lo = mid + 1; else hi = mid;
    }
    return false;
}

// Grid: blockIdx.x = query block * S + strip. A workgroup meets its rows in increasing order, so of two equal scores
// the one already in a list is the smaller row and stays ahead: a newcomer must beat the k-th entry strictly.
template <int MODE, int KL>
__global__ __launch_bounds__(256) void rank_tile_kernel(const float *__restrict__ q, long long Q,
                                                        const float *__restrict__ table, long long N, int D,
                                                        const float *__restrict__ rinv, const float *__restrict__ qinv,
                                                        const float *__restrict__ tsc, const int *__restrict__ trow,
                                                        const long long *__restrict__ off,
                                                        const long long *__restrict__ excl, long long E, int k, int S,
                                                        int tiles_per_strip, int *__restrict__ cnt,
                                                        float *__restrict__ cand_s, int *__restrict__ cand_r) {
    __shared__ __attribute__((aligned(16))) float smem[GT_SMEM_FLOATS];
    __shared__ float ls[GT_BM * KL];
    __shared__ int lr[GT_BM * KL];
    __shared__ int llen[GT_BM];
    const int t = threadIdx.x;
    const int strip = (int)(blockIdx.x % (unsigned)S);
    const long long q0 = (long long)(blockIdx.x / (unsigned)S) * GT_BM;
    if (t < GT_BM) llen[t] = 0;

    // the scan's view: 4 threads per query, 16 columns of the tile each
    const int srow = t >> 2, quarter = t & 3;
    const long long sq = q0 + srow;
    const bool svalid = sq < Q;
    const int tr = svalid ? trow[sq] : -1;
    const float ts = svalid ? tsc[sq] : 0.f;
    long long xlo = 0, xhi = 0;
    if (svalid && off) {
        xlo = off[sq];
        xhi = off[sq + 1];
        xlo = xlo < 0 ? 0 : (xlo > E ? E : xlo);
        xhi = xhi < xlo ? xlo : (xhi > E ? E : xhi);
    }
    // the epilogue's view: one column, 16 query rows
    float qv[16];
#pragma unroll
    for (int g = 0; g < 16; ++g) {
        const long long qi = q0 + acc_row(g);
        qv[g] = qi < Q ? qinv[qi] : 0.f;
    }
    const long long ar0 = q0 + stage_row(false, 0), ar1 = q0 + stage_row(false, 1);
    int count = 0;
    __syncthreads();

    for (int tile = 0; tile < tiles_per_strip; ++tile) {
        const long long c0 = ((long long)strip * tiles_per_strip + tile) * GT_BN;
        if (c0 >= N) break;
        RankLoader<MODE> L;
        L.init(q, table, D);
        const long long br0 = c0 + stage_row(false, 0), br1 = c0 + stage_row(false, 1);
        L.a0 = ar0 < Q;
        L.a1 = ar1 < Q;
        L.b0 = br0 < N;
        L.b1 = br1 < N;
        L.pa0 = q + (L.a0 ? ar0 : Q - 1) * D;
        L.pa1 = q + (L.a1 ? ar1 : Q - 1) * D;
        L.pb0 = table + (L.b0 ? br0 : N - 1) * D;
        L.pb1 = table + (L.b1 ? br1 : N - 1) * D;
        f32x16 acc;
#pragma unroll
        for (int g = 0; g < 16; ++g) acc[g] = 0.f;
        gemm_block<false, false>(acc, L, L.left, smem);         // (ends on a barrier: the LDS images are free)

        {
            const long long col = c0 + acc_col();
            const float rv = col < N ? rinv[col] : 0.f;
#pragma unroll
            for (int g = 0; g < 16; ++g) smem[acc_row(g) * RANK_TILE_LD + acc_col()] = rank_score(acc[g], rv, qv[g]);
        }
        __syncthreads();

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
                const bool in = svalid && col < N;
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
                        if (rank_excluded(excl, xlo, xhi, col)) continue;
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
    if (quarter == 0 && svalid && tr >= 0 && count) atomicAdd(&cnt[sq], count);
    for (int idx = t; idx < GT_BM * k; idx += 256) {
        const int row = idx / k, j = idx % k;
        const long long qi = q0 + row;
        if (qi >= Q) break;
        const bool have = j < llen[row];
        const long long dst = (qi * S + strip) * k + j;
        cand_s[dst] = have ? ls[row * KL + j] : -INFINITY;
        cand_r[dst] = have ? lr[row * KL + j] : -1;
    }
}

// ---------------------------------------------------------------------------------------------- merge
// One wave per query; lane l holds the head of strip l's list. Strips cover increasing rows, so on equal scores the
// lower lane is the smaller row.
__global__ __launch_bounds__(256) void rank_finish_kernel(long long Q, int k, int S, const float *__restrict__ cand_s,
                                                          const int *__restrict__ cand_r,
                                                          const float *__restrict__ tsc, const int *__restrict__ trow,
                                                          const int *__restrict__ cnt, const int *__restrict__ cntx,
                                                          long long *__restrict__ topk_rows,
                                                          float *__restrict__ topk_scores, long long *__restrict__ rank,
                                                          float *__restrict__ target_scores) {
    const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const bool live = i < Q;            // (no early return: every lane of the workgroup's waves meets the shuffles)
    if (live && lane == 0) {
        const int tr = trow[i];
        if (rank) rank[i] = tr >= 0 ? 1 + (long long)cnt[i] - (long long)cntx[i] : -1;
        if (target_scores) target_scores[i] = tr >= 0 ? tsc[i] : NAN;
    }
    const long long base = live && lane < S ? (i * S + lane) * k : -1;
    rank_merge_lists(live, lane, base, k, cand_s, cand_r, topk_rows + i * k, topk_scores + i * k);
}

// ---------------------------------------------------------------------------------------------- host
struct RankPlan {
    int S, tiles_per_strip;
    long long qblocks;
    size_t o_rinv, o_qinv, o_tsc, o_trow, o_cnt, o_cntx, o_cs, o_cr, bytes;
};

// Enough workgroups to fill the device about three times over, a strip never empty, at most one strip per merging lane.
static RankPlan rank_plan(int64_t Q, int64_t N, int k) {
    RankPlan p;
    p.qblocks = (Q + GT_BM - 1) / GT_BM;
    const long long tiles = (N + GT_BN - 1) / GT_BN;
    long long want = (768 + p.qblocks - 1) / p.qblocks;
    if (want > RANK_MAX_STRIPS) want = RANK_MAX_STRIPS;
    if (want > tiles) want = tiles;
    if (want < 1) want = 1;
    const long long tps = (tiles + want - 1) / want;
    p.tiles_per_strip = (int)tps;
    p.S = (int)((tiles + tps - 1) / tps);
    size_t o = 0;
    p.o_rinv = o; o += align_up((size_t)N * 4, 256);
    p.o_qinv = o; o += align_up((size_t)Q * 4, 256);
    p.o_tsc = o;  o += align_up((size_t)Q * 4, 256);
    p.o_trow = o; o += align_up((size_t)Q * 4, 256);
    p.o_cnt = o;  o += align_up((size_t)Q * 4, 256);
    p.o_cntx = o; o += align_up((size_t)Q * 4, 256);
    const size_t cand = (size_t)Q * (size_t)p.S * (size_t)(k > 0 ? k : 0) * 4;
    p.o_cs = o;   o += align_up(cand, 256);
    p.o_cr = o;   o += align_up(cand, 256);
    p.bytes = o + 256;
    return p;
}

static bool rank_shape_ok(int64_t Q, int64_t N, int64_t dim, int k) {
    const int64_t big = (int64_t)1 << 30;
    return Q <= big && N <= big && dim <= ((int64_t)1 << 20) && k <= RANK_MAX_K;
}

extern "C" size_t mpqe_rank_workspace_bytes(int64_t num_queries, int64_t table_rows, int64_t dim, int k) {
    if (num_queries < 1 || table_rows < 1 || dim <= 0 || k < 0 || !rank_shape_ok(num_queries, table_rows, dim, k)) return 0;
    return rank_plan(num_queries, table_rows, k).bytes;
}

template <int MODE>
static void rank_launch(const RankPlan &pl, const float *q, int64_t Q, const float *table, int64_t N, int D,
                        const int64_t *target_rows, const int64_t *off, const int64_t *excl, int64_t E, int k,
                        float *rinv, float *qinv, float *tsc, int *trow, int *cnt, int *cntx, float *cs, int *cr,
                        int32_t *err, hipStream_t s) {
    if (target_rows)
        hipLaunchKernelGGL(rank_pair_kernel<MODE>, dim3((unsigned)((Q + GT_BM - 1) / GT_BM)), dim3(256), 0, s, 0, q,
                           (long long)Q, table, (long long)N, D, (const float *)rinv, (const float *)qinv,
                           (const long long *)target_rows, (const long long *)off, (const long long *)excl,
                           (long long)E, tsc, trow, cntx, err);
    if (off && E > 0)       // (without targets too: this launch is also the one that checks the lists)
        hipLaunchKernelGGL(rank_pair_kernel<MODE>, dim3((unsigned)((E + GT_BM - 1) / GT_BM)), dim3(256), 0, s, 1, q,
                           (long long)Q, table, (long long)N, D, (const float *)rinv, (const float *)qinv,
                           (const long long *)target_rows, (const long long *)off, (const long long *)excl,
                           (long long)E, tsc, trow, cntx, err);
    const dim3 grid((unsigned)(pl.qblocks * pl.S));
    if (k <= RANK_SMALL_K)
        hipLaunchKernelGGL((rank_tile_kernel<MODE, RANK_SMALL_K>), grid, dim3(256), 0, s, q, (long long)Q, table,
                           (long long)N, D, (const float *)rinv, (const float *)qinv, (const float *)tsc,
                           (const int *)trow, (const long long *)off, (const long long *)excl, (long long)E, k, pl.S,
                           pl.tiles_per_strip, cnt, cs, cr);
    else if (k <= RANK_MID_K)
        hipLaunchKernelGGL((rank_tile_kernel<MODE, RANK_MID_K>), grid, dim3(256), 0, s, q, (long long)Q, table,
                           (long long)N, D, (const float *)rinv, (const float *)qinv, (const float *)tsc,
                           (const int *)trow, (const long long *)off, (const long long *)excl, (long long)E, k, pl.S,
                           pl.tiles_per_strip, cnt, cs, cr);
    else
        hipLaunchKernelGGL((rank_tile_kernel<MODE, RANK_MAX_K>), grid, dim3(256), 0, s, q, (long long)Q, table,
                           (long long)N, D, (const float *)rinv, (const float *)qinv, (const float *)tsc,
                           (const int *)trow, (const long long *)off, (const long long *)excl, (long long)E, k, pl.S,
                           pl.tiles_per_strip, cnt, cs, cr);
}

// score_kind 1: score(i, r) = q[i] . table[r], the pre-pass writing 1.0f for both factors. Nothing after the pre-pass
// knows a score's range: "no target" is trow < 0 and "no candidate" a row of -1 (the -inf beside them is never compared
// as a score of a live entry), lists are ordered by float compares, so finite scores of any size and sign rank alike.
extern "C" int mpqe_rank_entities_scored(const float *q, int64_t num_queries, const float *table, int64_t table_rows,
                                         int64_t dim, float eps, int score_kind, const int64_t *target_rows,
                                         const int64_t *excl_offsets, const int64_t *excl_rows, int64_t num_excluded, int k,
                                         int64_t *topk_rows, float *topk_scores, int64_t *rank, float *target_scores,
                                         void *workspace, size_t workspace_bytes, int32_t *err, void *stream) {
    const int64_t Q = num_queries, N = table_rows, E = num_excluded;
    if (Q < 0 || N < 1 || dim <= 0 || k < 0 || E < 0 || score_kind < 0 || score_kind > 1) return MPQE_ERR_INVALID_ARG;
    if (Q == 0) return MPQE_OK;
    if (!q || !table) return MPQE_ERR_INVALID_ARG;
    if (k > 0 && (!topk_rows || !topk_scores)) return MPQE_ERR_INVALID_ARG;
    if ((rank || target_scores) && !target_rows) return MPQE_ERR_INVALID_ARG;
    if ((E > 0 && (!excl_offsets || !excl_rows)) || (!excl_offsets && excl_rows)) return MPQE_ERR_INVALID_ARG;
    if (!rank_shape_ok(Q, N, dim, k)) return MPQE_ERR_UNSUPPORTED;
    const RankPlan pl = rank_plan(Q, N, k);
    if (!workspace || workspace_bytes < pl.bytes) return MPQE_ERR_WORKSPACE;
    char *w = reinterpret_cast<char *>(workspace);
    float *rinv = reinterpret_cast<float *>(w + pl.o_rinv), *qinv = reinterpret_cast<float *>(w + pl.o_qinv);
    float *tsc = reinterpret_cast<float *>(w + pl.o_tsc), *cs = reinterpret_cast<float *>(w + pl.o_cs);
    int *trow = reinterpret_cast<int *>(w + pl.o_trow), *cnt = reinterpret_cast<int *>(w + pl.o_cnt);
    int *cntx = reinterpret_cast<int *>(w + pl.o_cntx), *cr = reinterpret_cast<int *>(w + pl.o_cr);
    hipStream_t s = as_stream(stream);
    const int D = (int)dim;
    const int64_t *off = E > 0 ? excl_offsets : nullptr;        // (no entries: nothing is excluded)

    hipLaunchKernelGGL(rank_prep_kernel, dim3((unsigned)((N + Q + 3) / 4)), dim3(256), 0, s, q, (long long)Q, table,
                       (long long)N, D, eps, score_kind, rinv, qinv, tsc, trow, cnt, cntx);
    const bool vec = ptr_vec_ok(q, dim) && ptr_vec_ok(table, dim);
    if (vec && dim % GT_BK == 0)
        rank_launch<LD_FAST>(pl, q, Q, table, N, D, target_rows, off, excl_rows, E, k, rinv, qinv, tsc, trow, cnt, cntx,
                             cs, cr, err, s);
    else if (vec)
        rank_launch<LD_PRED>(pl, q, Q, table, N, D, target_rows, off, excl_rows, E, k, rinv, qinv, tsc, trow, cnt, cntx,
                             cs, cr, err, s);
    else
        rank_launch<LD_SCALAR>(pl, q, Q, table, N, D, target_rows, off, excl_rows, E, k, rinv, qinv, tsc, trow, cnt,
                               cntx, cs, cr, err, s);
    if (k > 0 || rank || target_scores)
        hipLaunchKernelGGL(rank_finish_kernel, dim3((unsigned)((Q + 3) / 4)), dim3(256), 0, s, (long long)Q, k, pl.S,
                           (const float *)cs, (const int *)cr, (const float *)tsc, (const int *)trow, (const int *)cnt,
                           (const int *)cntx, (long long *)topk_rows, topk_scores, (long long *)rank, target_scores);
    return mpqe_launch_status();
}

extern "C" int mpqe_rank_entities(const float *q, int64_t num_queries, const float *table, int64_t table_rows,
                                  int64_t dim, float eps, const int64_t *target_rows, const int64_t *excl_offsets,
                                  const int64_t *excl_rows, int64_t num_excluded, int k, int64_t *topk_rows,
                                  float *topk_scores, int64_t *rank, float *target_scores, void *workspace,
                                  size_t workspace_bytes, int32_t *err, void *stream) {
    return mpqe_rank_entities_scored(q, num_queries, table, table_rows, dim, eps, 0, target_rows, excl_offsets, excl_rows,
                                     num_excluded, k, topk_rows, topk_scores, rank, target_scores, workspace, workspace_bytes,
                                     err, stream);
}
