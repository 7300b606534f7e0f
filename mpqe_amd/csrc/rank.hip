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
// The kernels here are wrappers: rank_core.h holds the bodies that rank_mixed.hip (the queries of one call ranked against
// different tables) runs too -- the pre-pass's query branch, the gathered pair tile, the strip walk with its lists, the
// finishing wave, the strip rule and the launch dispatch. What is this file's own: a block's queries are q0 + j, a row is
// found excluded by a binary search of the query's sorted list at insertion time (rank_excluded), and the listed pairs'
// second mode counts the excluded rows that precede the target (cntx), which the finish takes out of the rank.
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
    if (i >= N) {
        rank_prep_query(q + (i - N) * D, D, lane, eps, score_kind, i - N, qinv, tsc, trow, cnt, cntx);
        return;
    }
    const float ss = rank_sumsq(table + i * D, D, lane, score_kind);
    if (lane != 0) return;
    rinv[i] = rank_row_inv(sqrtf(ss), score_kind);
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

// mode 0: pair p = (p, target_rows[p]); mode 1: pair p = (query of entry p, excl_rows[p]).
__device__ __forceinline__ RankPair rank_pair(int mode, long long p, long long Q, long long N,
                                              const long long *__restrict__ target_rows,
                                              const long long *__restrict__ off, const long long *__restrict__ excl,
                                              long long E) {
    RankPair P = {false, false, 0, 0};
    if (mode == 0) {
        if (p >= Q) return P;
        P.qi = p;
        P.r = target_rows[p];
    } else {
        if (p >= E) return P;
        P.qi = rank_entry_query(off, Q, p);
        if (off[P.qi] > p || off[P.qi + 1] <= p) return P;
        P.r = excl[p];
    }
    P.listed = true;
    P.ok = P.r >= 0 && P.r < N;
    return P;
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
    const RankPairDot d = rank_pair_tile<MODE>(
        q, table, D, [=](int j) { return rank_pair(mode, p0 + j, Q, N, target_rows, off, excl, E); }, smem, err);
    if (!d.mine) return;
    const long long p = p0 + acc_col(), qi = d.qi, r = d.r;
    const float s = rank_score(d.dot, rinv[r], qinv[qi]);
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

// The one-table view of the strip walk: block row j is query first + j; every row counts as it passes (the pair kernel's
// mode 1 takes the excluded ones out again) and the sorted list is searched only for a row about to enter a list.
struct RankOneTable : RankStrip {
    const long long *off, *excl;
    long long E, xlo, xhi;

    __device__ __forceinline__ long long query(int j) const { return first + j; }
    __device__ __forceinline__ void bind(bool ok, long long sq) {
        xlo = xhi = 0;
        if (ok && off) {
            xlo = off[sq];
            xhi = off[sq + 1];
            xlo = xlo < 0 ? 0 : (xlo > E ? E : xlo);
            xhi = xhi < xlo ? xlo : (xhi > E ? E : xhi);
        }
    }
    __device__ __forceinline__ unsigned out_mask(long long) const { return 0; }
    __device__ __forceinline__ bool excluded(long long col) const { return rank_excluded(excl, xlo, xhi, col); }
};

// Grid: blockIdx.x = query block * S + strip.
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
    RankOneTable V;
    V.q = q;
    V.table = table;
    V.rinv = rinv;
    V.qinv = qinv;
    V.tsc = tsc;
    V.trow = trow;
    V.cnt = cnt;
    V.cand_s = cand_s;
    V.cand_r = cand_r;
    V.N = N;
    V.first = (long long)(blockIdx.x / (unsigned)S) * GT_BM;
    V.D = D;
    V.k = k;
    V.live = Q - V.first < GT_BM ? (int)(Q - V.first) : GT_BM;
    V.S = S;
    V.tiles_per_strip = tiles_per_strip;
    V.strip = (int)(blockIdx.x % (unsigned)S);
    V.off = off;
    V.excl = excl;
    V.E = E;
    rank_strip_walk<MODE, KL>(V, smem, ls, lr, llen);
}

// ---------------------------------------------------------------------------------------------- merge
// One wave per query; lane l holds the head of strip l's list.
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
    rank_finish_wave(live, live, i, lane, live && lane < S ? (i * S + lane) * k : -1, k, cand_s, cand_r, tsc, trow, cnt,
                     cntx, topk_rows, topk_scores, rank, target_scores);
}

// ---------------------------------------------------------------------------------------------- host
struct RankPlan {
    int S, tiles_per_strip;
    long long qblocks;
    size_t o_rinv, o_qinv, o_tsc, o_trow, o_cnt, o_cntx, o_cs, o_cr, bytes;
};

static RankPlan rank_plan(int64_t Q, int64_t N, int k) {
    RankPlan p;
    p.qblocks = (Q + GT_BM - 1) / GT_BM;
    rank_strip_rule(p.qblocks, (N + GT_BN - 1) / GT_BN, p.S, p.tiles_per_strip);
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

struct RankArgs {
    const float *q, *table;
    long long Q, N, E;
    int D, k;
    const long long *target_rows, *off, *excl;
    float *rinv, *qinv, *tsc, *cs;
    int *trow, *cnt, *cntx, *cr;
    int32_t *err;
};

template <int MODE>
static void rank_launch_pairs(int mode, long long pairs, const RankArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(rank_pair_kernel<MODE>, dim3((unsigned)((pairs + GT_BM - 1) / GT_BM)), dim3(256), 0, s, mode, a.q,
                       a.Q, a.table, a.N, a.D, (const float *)a.rinv, (const float *)a.qinv, a.target_rows, a.off, a.excl,
                       a.E, a.tsc, a.trow, a.cntx, a.err);
}

template <int MODE>
static void rank_launch(const RankPlan &pl, const RankArgs &a, hipStream_t s) {
    if (a.target_rows) rank_launch_pairs<MODE>(0, a.Q, a, s);
    if (a.off && a.E > 0) rank_launch_pairs<MODE>(1, a.E, a, s);      // (without targets too: this launch checks the lists)
    rank_for_capacity(a.k, [&](auto kl) {
        hipLaunchKernelGGL((rank_tile_kernel<MODE, decltype(kl)::value>), dim3((unsigned)(pl.qblocks * pl.S)), dim3(256),
                           0, s, a.q, a.Q, a.table, a.N, a.D, (const float *)a.rinv, (const float *)a.qinv,
                           (const float *)a.tsc, (const int *)a.trow, a.off, a.excl, a.E, a.k, pl.S, pl.tiles_per_strip,
                           a.cnt, a.cs, a.cr);
    });
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
    RankArgs a;
    a.q = q;
    a.table = table;
    a.Q = Q;
    a.N = N;
    a.E = E;
    a.D = (int)dim;
    a.k = k;
    a.target_rows = (const long long *)target_rows;
    a.off = (const long long *)(E > 0 ? excl_offsets : nullptr);        // (no entries: nothing is excluded)
    a.excl = (const long long *)excl_rows;
    a.rinv = reinterpret_cast<float *>(w + pl.o_rinv);
    a.qinv = reinterpret_cast<float *>(w + pl.o_qinv);
    a.tsc = reinterpret_cast<float *>(w + pl.o_tsc);
    a.cs = reinterpret_cast<float *>(w + pl.o_cs);
    a.trow = reinterpret_cast<int *>(w + pl.o_trow);
    a.cnt = reinterpret_cast<int *>(w + pl.o_cnt);
    a.cntx = reinterpret_cast<int *>(w + pl.o_cntx);
    a.cr = reinterpret_cast<int *>(w + pl.o_cr);
    a.err = err;
    hipStream_t s = as_stream(stream);

    hipLaunchKernelGGL(rank_prep_kernel, dim3((unsigned)((N + Q + 3) / 4)), dim3(256), 0, s, q, a.Q, table, a.N, a.D, eps,
                       score_kind, a.rinv, a.qinv, a.tsc, a.trow, a.cnt, a.cntx);
    rank_for_load_mode(ptr_vec_ok(q, dim) && ptr_vec_ok(table, dim), dim,
                       [&](auto mode) { rank_launch<decltype(mode)::value>(pl, a, s); });
    if (k > 0 || rank || target_scores)
        hipLaunchKernelGGL(rank_finish_kernel, dim3((unsigned)((Q + 3) / 4)), dim3(256), 0, s, a.Q, k, pl.S,
                           (const float *)a.cs, (const int *)a.cr, (const float *)a.tsc, (const int *)a.trow,
                           (const int *)a.cnt, (const int *)a.cntx, (long long *)topk_rows, topk_scores,
                           (long long *)rank, target_scores);
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
