// Ranking the queries of ONE call against DIFFERENT tables: query i is ranked against candidate set
// set_of_group[group_of[i]] (the entities of its formula's target mode), with the score, the total order, the integer
// counters and the strip lists of rank.hip (rank_core.h holds what both files run). Every rank, top-k row and score and
// target score equals bit for bit what mpqe_rank_entities_scored gives the queries of one set handed to it alone.
//
// The sets live in a descriptor block the caller keeps (mpqe_rank_mixed_desc_build: addresses, sizes, score kinds and the
// group -> set table; nothing per call). Five launches, none waits for a workgroup of its own launch:
//   rmx_plan_kernel     one workgroup: the set of every query, a stable sort of the queries by set (kg_scan.h's scan over
//                       per-thread counts, one pass per set) and the table of 64-query blocks (set, first position, count).
//                       At most Q/64 + num_sets blocks: the later grids are sized to that bound and spare workgroups leave.
//   rmx_prep_kernel     1/|row| of every set's rows, 1/max(|q|, eps) per query by its set's score kind; counters zeroed
//   rmx_pair_kernel     the targets' scores as the diagonal of a gathered tile (rank.hip's mode 0)
//   rmx_tile_kernel     a block's queries (read through the permutation) x a strip of its set's tiles; a row is eligible
//                       when its bit in the set's `valid` words is set and its bit in the query's exclusion words is clear:
//                       a thread tests 16 columns against one word of each, so ineligible rows are left out of the count
//                       as they pass and rank.hip's pass over exclusion lists (mode 1) has no counterpart
//   rmx_finish_kernel   one wave per sorted position: merges the strip lists, writes the query's outputs
// The strip count S comes from the widest set; a narrower set spreads its own tiles over the same S strips. Per-query
// state lives where rank.hip keeps it (threshold, target and masks in registers, the k-lists in LDS beside the tile
// image), so the LDS per workgroup and the occupancy are rank.hip's.
#include <string.h>

#include <new>

#include "kg_scan.h"
#include "rank_core.h"

#define RMX_MAX_SETS 256
#define RMX_MAX_GROUPS (1 << 20)

struct RmxHdr {
    long long total_rows, max_rows;
    int num_sets, num_groups;
    int pad[10];
};
struct RmxSet {
    const float *table;
    const uint32_t *valid;
    long long rows, first;          // first: the set's offset among all sets' rows (its 1/|row| values start there)
    int kind, pad;
};
struct RmxBlock {
    int set, first, count, pad;
};
struct RmxState {                   // the first words of the workspace
    int nblocks, ngood;
};

static inline size_t rmx_sets_bytes(int64_t num_sets) {
    return align_up(sizeof(RmxHdr) + (size_t)num_sets * sizeof(RmxSet), 256);
}
__host__ __device__ __forceinline__ const RmxSet *rmx_sets(const void *desc) {
    return reinterpret_cast<const RmxSet *>(reinterpret_cast<const char *>(desc) + sizeof(RmxHdr));
}
// The block was built for these counts (a call that names other ones ranks nothing: its sizes were not the block's).
__device__ __forceinline__ bool rmx_desc_matches(const void *desc, int num_sets, int num_groups, long long max_rows,
                                                 long long total_rows) {
    const RmxHdr *h = reinterpret_cast<const RmxHdr *>(desc);
    return h->num_sets == num_sets && h->num_groups == num_groups && h->max_rows == max_rows &&
           h->total_rows == total_rows;
}

// ---------------------------------------------------------------------------------------------- plan
// One workgroup. Thread t owns the queries [t * chunk, (t + 1) * chunk): a pass per set counts its queries of that set,
// the scan places them behind the lower threads', so equal sets keep the queries' order. The bad ones (group out of
// range) are the last pass: they get positions too, behind ngood, and no block.
__global__ __launch_bounds__(256) void rmx_plan_kernel(const void *__restrict__ desc, const int *__restrict__ set_of_group,
                                                       int num_sets, int num_groups, long long max_rows,
                                                       long long total_rows, const long long *__restrict__ group_of,
                                                       int Q, int *__restrict__ qset, int *__restrict__ perm,
                                                       RmxBlock *__restrict__ blocks, RmxState *__restrict__ state,
                                                       int32_t *err) {
    __shared__ int wsum[KG_SCAN_WAVES];
    const int t = threadIdx.x;
    const bool match = rmx_desc_matches(desc, num_sets, num_groups, max_rows, total_rows);
    const int chunk = (Q + 255) / 256;
    const long long lo_ = (long long)t * chunk, hi_ = lo_ + chunk;
    const int lo = (int)(lo_ < Q ? lo_ : Q), hi = (int)(hi_ < Q ? hi_ : Q);
    bool bad = !match && t == 0;
    for (int i = lo; i < hi; ++i) {
        const long long g = group_of[i];
        int s = num_sets;
        if (match && g >= 0 && g < num_groups) {
            s = set_of_group[g];
            if (s < 0 || s >= num_sets) s = num_sets;
        }
        bad |= s == num_sets;
        qset[i] = s;
    }
    if (bad) flag_error(err, MPQE_FLAG_BAD_INDEX);
    int base = 0, blk = 0;
    for (int s = 0; s <= num_sets; ++s) {
        int mine = 0;
        for (int i = lo; i < hi; ++i) mine += qset[i] == s ? 1 : 0;
        int total;
        int p = base + kg_workgroup_scan(mine, wsum, total);
        for (int i = lo; i < hi; ++i)
            if (qset[i] == s) perm[p++] = i;
        if (s < num_sets) {
            const int nb = (total + GT_BM - 1) / GT_BM;
            for (int b = t; b < nb; b += 256) {
                RmxBlock B;
                B.set = s;
                B.first = base + b * GT_BM;
                B.count = total - b * GT_BM < GT_BM ? total - b * GT_BM : GT_BM;
                B.pad = 0;
                blocks[blk + b] = B;
            }
            blk += nb;
        } else if (t == 0) {
            state->nblocks = blk;
            state->ngood = base;
        }
        base += total;
        __syncthreads();            // (the next pass's scan rewrites wsum)
    }
}

// ---------------------------------------------------------------------------------------------- pre-pass
__global__ __launch_bounds__(256) void rmx_prep_kernel(const void *__restrict__ desc, int num_sets, int num_groups,
                                                       long long max_rows, long long total_rows,
                                                       const float *__restrict__ q, long long Q, int D, float eps,
                                                       const int *__restrict__ qset, float *__restrict__ rinv,
                                                       float *__restrict__ qinv, float *__restrict__ tsc,
                                                       int *__restrict__ trow, int *__restrict__ cnt) {
    const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= total_rows + Q) return;
    const int lane = threadIdx.x & 63;
    const RmxSet *sets = rmx_sets(desc);
    if (i >= total_rows) {
        const long long j = i - total_rows;
        const int s = qset[j];
        const int kind = s < num_sets ? sets[s].kind : 1;       // (a query without a set: nothing reads its factor)
        const float ss = rank_sumsq(q + j * D, D, lane, kind);
        if (lane != 0) return;
        qinv[j] = rank_query_inv(sqrtf(ss), eps, kind);
        tsc[j] = -INFINITY;
        trow[j] = -1;
        cnt[j] = 0;
        return;
    }
    if (!rmx_desc_matches(desc, num_sets, num_groups, max_rows, total_rows)) return;
    int a = 0, b = num_sets - 1;        // the last set that starts at or before row i
    while (a < b) {
        const int mid = (a + b + 1) >> 1;
        if (sets[mid].first <= i) a = mid; else b = mid - 1;
    }
    const RmxSet S = sets[a];
    const long long r = i - S.first;
    if (r < 0 || r >= S.rows) return;
    const float ss = rank_sumsq(S.table + r * D, D, lane, S.kind);
    if (lane != 0) return;
    rinv[i] = rank_row_inv(sqrtf(ss), S.kind);
}

// ---------------------------------------------------------------------------------------------- targets
// Pair j of block b = (the query at position first + j, its target row) against the block's set.
__device__ __forceinline__ bool rmx_pair(const RmxBlock &B, long long N, int j, const int *__restrict__ perm,
                                         const long long *__restrict__ target_rows, long long &qi, long long &r,
                                         bool &listed) {
    listed = j < B.count;
    qi = 0;
    r = 0;
    if (!listed) return false;
    qi = perm[B.first + j];
    r = target_rows[qi];
    return r >= 0 && r < N;
}

template <int MODE>
__global__ __launch_bounds__(256) void rmx_pair_kernel(const void *__restrict__ desc, const RmxBlock *__restrict__ blocks,
                                                       const RmxState *__restrict__ state, const int *__restrict__ perm,
                                                       const float *__restrict__ q, int D,
                                                       const float *__restrict__ rinv, const float *__restrict__ qinv,
                                                       const long long *__restrict__ target_rows,
                                                       float *__restrict__ tsc, int *__restrict__ trow, int32_t *err) {
    __shared__ __attribute__((aligned(16))) float smem[GT_SMEM_FLOATS];
    if ((int)blockIdx.x >= state->nblocks) return;
    const RmxBlock B = blocks[blockIdx.x];
    const RmxSet S = rmx_sets(desc)[B.set];
    const long long N = S.rows;
    RankLoader<MODE> L;
    L.init(q, S.table, D);
    {
        long long qi, r;
        bool listed;
        bool ok = rmx_pair(B, N, stage_row(false, 0), perm, target_rows, qi, r, listed);
        L.a0 = L.b0 = ok;
        L.pa0 = q + (ok ? qi : 0) * D;
        L.pb0 = S.table + (ok ? r : 0) * D;
        ok = rmx_pair(B, N, stage_row(false, 1), perm, target_rows, qi, r, listed);
        L.a1 = L.b1 = ok;
        L.pa1 = q + (ok ? qi : 0) * D;
        L.pb1 = S.table + (ok ? r : 0) * D;
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
    long long qi, r;
    bool listed;
    const bool ok = rmx_pair(B, N, col, perm, target_rows, qi, r, listed);
    if (!listed) return;
    if (!ok) {
        flag_error(err, MPQE_FLAG_BAD_INDEX);       // (the pre-pass left "no target" for this query)
        return;
    }
    tsc[qi] = rank_score(dot, rinv[S.first + r], qinv[qi]);
    trow[qi] = (int)r;
}

// ---------------------------------------------------------------------------------------------- all rows
// Grid: blockIdx.x = block * S + strip. As rank_tile_kernel: a workgroup meets its rows in increasing order, so of two
// equal scores the one already in a list is the smaller row and stays ahead.
template <int MODE, int KL>
__global__ __launch_bounds__(256) void rmx_tile_kernel(const void *__restrict__ desc, const RmxBlock *__restrict__ blocks,
                                                       const RmxState *__restrict__ state, const int *__restrict__ perm,
                                                       const float *__restrict__ q, int D,
                                                       const float *__restrict__ rinv_all, const float *__restrict__ qinv,
                                                       const float *__restrict__ tsc, const int *__restrict__ trow,
                                                       const int32_t *__restrict__ excl_bits, long long W, int k, int S,
                                                       int *__restrict__ cnt, float *__restrict__ cand_s,
                                                       int *__restrict__ cand_r) {
    __shared__ __attribute__((aligned(16))) float smem[GT_SMEM_FLOATS];
    __shared__ float ls[GT_BM * KL];
    __shared__ int lr[GT_BM * KL];
    __shared__ int llen[GT_BM];
    const int t = threadIdx.x;
    const int strip = (int)(blockIdx.x % (unsigned)S);
    const int block = (int)(blockIdx.x / (unsigned)S);
    if (block >= state->nblocks) return;
    const RmxBlock B = blocks[block];
    const RmxSet St = rmx_sets(desc)[B.set];
    const long long N = St.rows;
    const float *table = St.table;
    const float *rinv = rinv_all + St.first;
    const int tiles = (int)((N + GT_BN - 1) / GT_BN);
    const int tiles_per_strip = (tiles + S - 1) / S;
    if (t < GT_BM) llen[t] = 0;

    // the scan's view: 4 threads per query, 16 columns of the tile each
    const int srow = t >> 2, quarter = t & 3;
    const bool svalid = srow < B.count;
    const long long sq = svalid ? perm[B.first + srow] : 0;
    const int tr = svalid ? trow[sq] : -1;
    const float ts = svalid ? tsc[sq] : 0.f;
    const uint32_t *xw = svalid && excl_bits ? reinterpret_cast<const uint32_t *>(excl_bits) + sq * W : nullptr;
    // the epilogue's view: one column, 16 query rows
    float qv[16];
#pragma unroll
    for (int g = 0; g < 16; ++g) {
        const int row = acc_row(g);
        qv[g] = row < B.count ? qinv[perm[B.first + row]] : 0.f;
    }
    const int a0 = stage_row(false, 0), a1 = stage_row(false, 1);
    const long long ar0 = perm[B.first + (a0 < B.count ? a0 : 0)], ar1 = perm[B.first + (a1 < B.count ? a1 : 0)];
    int count = 0;
    __syncthreads();

    for (int tile = 0; tile < tiles_per_strip; ++tile) {
        const long long c0 = ((long long)strip * tiles_per_strip + tile) * GT_BN;
        if (c0 >= N) break;
        RankLoader<MODE> L;
        L.init(q, table, D);
        const long long br0 = c0 + stage_row(false, 0), br1 = c0 + stage_row(false, 1);
        L.a0 = a0 < B.count;
        L.a1 = a1 < B.count;
        L.b0 = br0 < N;
        L.b1 = br1 < N;
        L.pa0 = q + ar0 * D;                // (a row past the block: the block's first query, its result is not used)
        L.pa1 = q + ar1 * D;
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

        // this thread's 16 columns lie in one 32-bit word of either bitmap: bit j of `out` set = column j not eligible
        unsigned out = 0;
        {
            const long long cq = c0 + quarter * 16;
            const long long word = cq >> 5;
            const int shift = (int)(cq & 31);
            if (xw && word < W) out |= xw[word] >> shift;
            if (St.valid && cq < N) out |= ~(St.valid[word] >> shift);
            out &= 0xffffu;
        }
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
                if (svalid && col < N && tr >= 0 && col != tr && !(out & (1u << j)) &&
                    (s > ts || (s == ts && col < tr)))
                    ++count;
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
                        llen[srow] = rank_list_insert(S_, R_, len, k, s, (int)(c0 + quarter * 16 + j));
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
        if (row >= B.count) break;
        const bool have = j < llen[row];
        const long long dst = ((long long)(B.first + row) * S + strip) * k + j;
        cand_s[dst] = have ? ls[row * KL + j] : -INFINITY;
        cand_r[dst] = have ? lr[row * KL + j] : -1;
    }
}

// ---------------------------------------------------------------------------------------------- merge
// One wave per sorted position p; the outputs go to the query that sits there. A position at or behind ngood holds a
// query without a set: no list, no target.
__global__ __launch_bounds__(256) void rmx_finish_kernel(long long Q, int k, int S, const RmxState *__restrict__ state,
                                                         const int *__restrict__ perm, const float *__restrict__ cand_s,
                                                         const int *__restrict__ cand_r, const float *__restrict__ tsc,
                                                         const int *__restrict__ trow, const int *__restrict__ cnt,
                                                         long long *__restrict__ topk_rows,
                                                         float *__restrict__ topk_scores, long long *__restrict__ rank,
                                                         float *__restrict__ target_scores) {
    const long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const bool live = p < Q;            // (no early return: every lane of the workgroup's waves meets the shuffles)
    const bool good = live && p < state->ngood;
    const long long i = live ? perm[p] : 0;
    if (live && lane == 0) {
        const int tr = good ? trow[i] : -1;
        if (rank) rank[i] = tr >= 0 ? 1 + (long long)cnt[i] : -1;
        if (target_scores) target_scores[i] = tr >= 0 ? tsc[i] : NAN;
    }
    const long long base = good && lane < S ? (p * S + lane) * k : -1;
    rank_merge_lists(live, lane, base, k, cand_s, cand_r, topk_rows + i * k, topk_scores + i * k);
}

// ---------------------------------------------------------------------------------------------- host
static inline bool rmx_counts_ok(int64_t num_sets, int64_t num_groups) {
    return num_sets >= 1 && num_sets <= RMX_MAX_SETS && num_groups >= 1 && num_groups <= RMX_MAX_GROUPS;
}
static inline size_t rmx_desc_size(int64_t num_sets, int64_t num_groups) {
    return rmx_sets_bytes(num_sets) + align_up((size_t)num_groups * 4, 256);
}

extern "C" size_t mpqe_rank_mixed_desc_bytes(int64_t num_sets, int64_t num_groups) {
    return rmx_counts_ok(num_sets, num_groups) ? rmx_desc_size(num_sets, num_groups) : 0;
}

extern "C" int mpqe_rank_mixed_desc_build(const float *const *tables_host, const int64_t *rows_host,
                                          const int32_t *kinds_host, const uint32_t *const *valid_host, int64_t num_sets,
                                          const int32_t *set_of_group_host, int64_t num_groups, void *desc,
                                          size_t desc_bytes, void *stream) {
    if (!rmx_counts_ok(num_sets, num_groups)) return MPQE_ERR_INVALID_ARG;
    if (!tables_host || !rows_host || !kinds_host || !set_of_group_host || !desc) return MPQE_ERR_INVALID_ARG;
    if ((uintptr_t)desc % 256 != 0) return MPQE_ERR_INVALID_ARG;
    const int64_t big = (int64_t)1 << 30;
    int64_t total = 0, widest = 0;
    for (int64_t s = 0; s < num_sets; ++s) {
        if (!tables_host[s] || rows_host[s] < 1 || rows_host[s] > big) return MPQE_ERR_INVALID_ARG;
        if (kinds_host[s] < 0 || kinds_host[s] > 1) return MPQE_ERR_INVALID_ARG;
        if ((uintptr_t)tables_host[s] % 16 != 0) return MPQE_ERR_UNSUPPORTED;
        if (valid_host && valid_host[s] && (uintptr_t)valid_host[s] % 4 != 0) return MPQE_ERR_INVALID_ARG;
        total += rows_host[s];
        widest = rows_host[s] > widest ? rows_host[s] : widest;
    }
    if (total > big) return MPQE_ERR_UNSUPPORTED;
    for (int64_t g = 0; g < num_groups; ++g)
        if (set_of_group_host[g] < 0 || set_of_group_host[g] >= num_sets) return MPQE_ERR_INVALID_ARG;
    const size_t need = rmx_desc_size(num_sets, num_groups), head = rmx_sets_bytes(num_sets);
    if (desc_bytes < need) return MPQE_ERR_WORKSPACE;
    char *image = new (std::nothrow) char[need];
    if (!image) return MPQE_ERR_INVALID_ARG;
    memset(image, 0, need);
    RmxHdr *h = reinterpret_cast<RmxHdr *>(image);
    h->total_rows = total;
    h->max_rows = widest;
    h->num_sets = (int)num_sets;
    h->num_groups = (int)num_groups;
    RmxSet *sets = reinterpret_cast<RmxSet *>(image + sizeof(RmxHdr));
    long long first = 0;
    for (int64_t s = 0; s < num_sets; ++s) {
        sets[s].table = tables_host[s];
        sets[s].valid = valid_host ? valid_host[s] : nullptr;
        sets[s].rows = rows_host[s];
        sets[s].first = first;
        sets[s].kind = kinds_host[s];
        first += rows_host[s];
    }
    memcpy(image + head, set_of_group_host, (size_t)num_groups * 4);
    int st = MPQE_OK;
    if (hipMemcpyAsync(desc, image, need, hipMemcpyHostToDevice, as_stream(stream)) != hipSuccess) st = MPQE_ERR_LAUNCH;
    // (the copy reads pageable memory: it has left `image` when the call returns)
    delete[] image;
    return st;
}

struct RmxPlan {
    int S;
    long long max_blocks;
    size_t o_state, o_qset, o_perm, o_blocks, o_rinv, o_qinv, o_tsc, o_trow, o_cnt, o_cs, o_cr, bytes;
};

// rank.hip's rule for the strip count, on the bound of the block count and the widest set's tiles.
static RmxPlan rmx_plan(int64_t Q, int64_t num_sets, int64_t max_rows, int64_t total_rows, int k) {
    RmxPlan p;
    p.max_blocks = Q / GT_BM + num_sets;
    const long long tiles = (max_rows + GT_BN - 1) / GT_BN;
    long long want = (768 + p.max_blocks - 1) / p.max_blocks;
    if (want > RANK_MAX_STRIPS) want = RANK_MAX_STRIPS;
    if (want > tiles) want = tiles;
    if (want < 1) want = 1;
    const long long tps = (tiles + want - 1) / want;
    p.S = (int)((tiles + tps - 1) / tps);
    size_t o = 0;
    p.o_state = o;  o += 256;
    p.o_qset = o;   o += align_up((size_t)Q * 4, 256);
    p.o_perm = o;   o += align_up((size_t)Q * 4, 256);
    p.o_blocks = o; o += align_up((size_t)p.max_blocks * sizeof(RmxBlock), 256);
    p.o_rinv = o;   o += align_up((size_t)total_rows * 4, 256);
    p.o_qinv = o;   o += align_up((size_t)Q * 4, 256);
    p.o_tsc = o;    o += align_up((size_t)Q * 4, 256);
    p.o_trow = o;   o += align_up((size_t)Q * 4, 256);
    p.o_cnt = o;    o += align_up((size_t)Q * 4, 256);
    const size_t cand = (size_t)Q * (size_t)p.S * (size_t)(k > 0 ? k : 0) * 4;
    p.o_cs = o;     o += align_up(cand, 256);
    p.o_cr = o;     o += align_up(cand, 256);
    p.bytes = o;
    return p;
}

static bool rmx_shape_ok(int64_t Q, int64_t num_sets, int64_t max_rows, int64_t total_rows, int64_t dim, int k) {
    const int64_t big = (int64_t)1 << 30;
    return Q <= big && num_sets <= RMX_MAX_SETS && total_rows <= big && dim <= ((int64_t)1 << 20) && k <= RANK_MAX_K &&
           max_rows <= total_rows && total_rows <= max_rows * num_sets;
}

extern "C" size_t mpqe_rank_mixed_workspace_bytes(int64_t num_queries, int64_t num_sets, int64_t max_rows,
                                                  int64_t total_rows, int64_t dim, int k) {
    if (num_queries < 1 || num_sets < 1 || max_rows < 1 || total_rows < 1 || dim <= 0 || k < 0) return 0;
    if (!rmx_shape_ok(num_queries, num_sets, max_rows, total_rows, dim, k)) return 0;
    return rmx_plan(num_queries, num_sets, max_rows, total_rows, k).bytes;
}

struct RmxArgs {
    const void *desc;
    const RmxBlock *blocks;
    const RmxState *state;
    const int *perm;
    const float *q;
    int D;
    float *rinv, *qinv, *tsc;
    int *trow, *cnt;
    float *cs;
    int *cr;
    const int64_t *target_rows;
    const int32_t *excl_bits;
    int64_t W;
    int k;
    int32_t *err;
};

template <int MODE>
static void rmx_launch(const RmxPlan &pl, const RmxArgs &a, hipStream_t s) {
    if (a.target_rows)
        hipLaunchKernelGGL(rmx_pair_kernel<MODE>, dim3((unsigned)pl.max_blocks), dim3(256), 0, s, a.desc, a.blocks,
                           a.state, a.perm, a.q, a.D, (const float *)a.rinv, (const float *)a.qinv,
                           (const long long *)a.target_rows, a.tsc, a.trow, a.err);
    const dim3 grid((unsigned)(pl.max_blocks * pl.S));
    if (a.k <= RANK_SMALL_K)
        hipLaunchKernelGGL((rmx_tile_kernel<MODE, RANK_SMALL_K>), grid, dim3(256), 0, s, a.desc, a.blocks, a.state, a.perm,
                           a.q, a.D, (const float *)a.rinv, (const float *)a.qinv, (const float *)a.tsc,
                           (const int *)a.trow, a.excl_bits, (long long)a.W, a.k, pl.S, a.cnt, a.cs, a.cr);
    else if (a.k <= RANK_MID_K)
        hipLaunchKernelGGL((rmx_tile_kernel<MODE, RANK_MID_K>), grid, dim3(256), 0, s, a.desc, a.blocks, a.state, a.perm,
                           a.q, a.D, (const float *)a.rinv, (const float *)a.qinv, (const float *)a.tsc,
                           (const int *)a.trow, a.excl_bits, (long long)a.W, a.k, pl.S, a.cnt, a.cs, a.cr);
    else
        hipLaunchKernelGGL((rmx_tile_kernel<MODE, RANK_MAX_K>), grid, dim3(256), 0, s, a.desc, a.blocks, a.state, a.perm,
                           a.q, a.D, (const float *)a.rinv, (const float *)a.qinv, (const float *)a.tsc,
                           (const int *)a.trow, a.excl_bits, (long long)a.W, a.k, pl.S, a.cnt, a.cs, a.cr);
}

extern "C" int mpqe_rank_entities_mixed(const float *q, int64_t num_queries, int64_t dim, float eps, const void *desc,
                                        size_t desc_bytes, int64_t num_sets, int64_t num_groups, int64_t max_rows,
                                        int64_t total_rows, const int64_t *group_of, const int64_t *target_rows,
                                        const int32_t *excl_bits, int64_t excl_stride_words, int k, int64_t *topk_rows,
                                        float *topk_scores, int64_t *rank, float *target_scores, void *workspace,
                                        size_t workspace_bytes, int32_t *err, void *stream) {
    const int64_t Q = num_queries;
    if (Q < 0 || dim <= 0 || k < 0 || max_rows < 1 || total_rows < 1) return MPQE_ERR_INVALID_ARG;
    if (!rmx_counts_ok(num_sets, num_groups)) return MPQE_ERR_INVALID_ARG;
    if (Q == 0) return MPQE_OK;
    if (!q || !desc || !group_of) return MPQE_ERR_INVALID_ARG;
    if ((uintptr_t)desc % 256 != 0) return MPQE_ERR_INVALID_ARG;
    if (k > 0 && (!topk_rows || !topk_scores)) return MPQE_ERR_INVALID_ARG;
    if ((rank || target_scores) && !target_rows) return MPQE_ERR_INVALID_ARG;
    if (excl_bits && excl_stride_words < 1) return MPQE_ERR_INVALID_ARG;
    if (!rmx_shape_ok(Q, num_sets, max_rows, total_rows, dim, k)) return MPQE_ERR_UNSUPPORTED;
    if (desc_bytes < rmx_desc_size(num_sets, num_groups)) return MPQE_ERR_WORKSPACE;
    const RmxPlan pl = rmx_plan(Q, num_sets, max_rows, total_rows, k);
    if (!workspace || workspace_bytes < pl.bytes) return MPQE_ERR_WORKSPACE;
    if ((uintptr_t)workspace % 256 != 0) return MPQE_ERR_INVALID_ARG;
    char *w = reinterpret_cast<char *>(workspace);
    RmxState *state = reinterpret_cast<RmxState *>(w + pl.o_state);
    int *qset = reinterpret_cast<int *>(w + pl.o_qset), *perm = reinterpret_cast<int *>(w + pl.o_perm);
    RmxBlock *blocks = reinterpret_cast<RmxBlock *>(w + pl.o_blocks);
    RmxArgs a;
    a.desc = desc;
    a.blocks = blocks;
    a.state = state;
    a.perm = perm;
    a.q = q;
    a.D = (int)dim;
    a.rinv = reinterpret_cast<float *>(w + pl.o_rinv);
    a.qinv = reinterpret_cast<float *>(w + pl.o_qinv);
    a.tsc = reinterpret_cast<float *>(w + pl.o_tsc);
    a.trow = reinterpret_cast<int *>(w + pl.o_trow);
    a.cnt = reinterpret_cast<int *>(w + pl.o_cnt);
    a.cs = reinterpret_cast<float *>(w + pl.o_cs);
    a.cr = reinterpret_cast<int *>(w + pl.o_cr);
    a.target_rows = target_rows;
    a.excl_bits = excl_bits;
    a.W = excl_bits ? excl_stride_words : 0;
    a.k = k;
    a.err = err;
    hipStream_t s = as_stream(stream);
    const int *set_of_group =
        reinterpret_cast<const int *>(reinterpret_cast<const char *>(desc) + rmx_sets_bytes(num_sets));

    hipLaunchKernelGGL(rmx_plan_kernel, dim3(1), dim3(256), 0, s, desc, set_of_group, (int)num_sets, (int)num_groups,
                       (long long)max_rows, (long long)total_rows, (const long long *)group_of, (int)Q, qset, perm, blocks,
                       state, err);
    hipLaunchKernelGGL(rmx_prep_kernel, dim3((unsigned)((total_rows + Q + 3) / 4)), dim3(256), 0, s, desc, (int)num_sets,
                       (int)num_groups, (long long)max_rows, (long long)total_rows, q, (long long)Q, a.D, eps,
                       (const int *)qset, a.rinv, a.qinv, a.tsc, a.trow, a.cnt);
    // (the tables' rows are 16-byte aligned by the descriptor's build: the load mode hangs on q and dim alone)
    const bool vec = ptr_vec_ok(q, dim);
    if (vec && dim % GT_BK == 0)
        rmx_launch<LD_FAST>(pl, a, s);
    else if (vec)
        rmx_launch<LD_PRED>(pl, a, s);
    else
        rmx_launch<LD_SCALAR>(pl, a, s);
    if (k > 0 || rank || target_scores)
        hipLaunchKernelGGL(rmx_finish_kernel, dim3((unsigned)((Q + 3) / 4)), dim3(256), 0, s, (long long)Q, k, pl.S,
                           (const RmxState *)state, (const int *)perm, (const float *)a.cs, (const int *)a.cr,
                           (const float *)a.tsc, (const int *)a.trow, (const int *)a.cnt, (long long *)topk_rows,
                           topk_scores, (long long *)rank, target_scores);
    return mpqe_launch_status();
}
