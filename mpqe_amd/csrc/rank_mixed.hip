// Ranking the queries of ONE call against DIFFERENT tables: query i is ranked against candidate set
// set_of_group[group_of[i]] (the entities of its formula's target mode), with the score, the total order, the integer
// counters and the strip lists of rank.hip. Every rank, top-k row and score and target score equals bit for bit what
// mpqe_rank_entities_scored gives the queries of one set handed to it alone: the pre-pass's query branch, the pair tile,
// the strip walk, the finishing wave and the strip rule are rank_core.h's one definition each, and the kernels below are
// wrappers that read the block and set records, fill in the walk's view (RmxStrip: the permutation and the two bitmaps)
// and call them.
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
        rank_prep_query(q + j * D, D, lane, eps, kind, j, qinv, tsc, trow, cnt, nullptr);
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
    const RankPairDot d = rank_pair_tile<MODE>(
        q, S.table, D,
        [=](int j) {
            RankPair P = {j < B.count, false, 0, 0};
            if (!P.listed) return P;
            P.qi = perm[B.first + j];
            P.r = target_rows[P.qi];
            P.ok = P.r >= 0 && P.r < S.rows;
            return P;
        },
        smem, err);
    if (!d.mine) return;
    tsc[d.qi] = rank_score(d.dot, rinv[S.first + d.r], qinv[d.qi]);
    trow[d.qi] = (int)d.r;
}

// ---------------------------------------------------------------------------------------------- all rows
// The mixed view of the strip walk: block row j is the query at sorted position first + j; this thread's 16 columns lie
// in one 32-bit word of either bitmap, so a row that is not eligible is left out of the count as it passes and nothing
// is left to ask at insertion time.
struct RmxStrip : RankStrip {
    const int *perm;
    const uint32_t *valid, *xbits, *xw;
    long long W;

    __device__ __forceinline__ long long query(int j) const { return perm[first + j]; }
    __device__ __forceinline__ void bind(bool ok, long long sq) { xw = ok && xbits ? xbits + sq * W : nullptr; }
    __device__ __forceinline__ unsigned out_mask(long long cq) const {
        const long long word = cq >> 5;
        const int shift = (int)(cq & 31);
        unsigned out = 0;
        if (xw && word < W) out |= xw[word] >> shift;
        if (valid && cq < N) out |= ~(valid[word] >> shift);
        return out & 0xffffu;
    }
    __device__ __forceinline__ bool excluded(long long) const { return false; }
};

// Grid: blockIdx.x = block * S + strip.
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
    const int block = (int)(blockIdx.x / (unsigned)S);
    if (block >= state->nblocks) return;
    const RmxBlock B = blocks[block];
    const RmxSet St = rmx_sets(desc)[B.set];
    RmxStrip V;
    V.q = q;
    V.table = St.table;
    V.rinv = rinv_all + St.first;
    V.qinv = qinv;
    V.tsc = tsc;
    V.trow = trow;
    V.cnt = cnt;
    V.cand_s = cand_s;
    V.cand_r = cand_r;
    V.N = St.rows;
    V.first = B.first;
    V.D = D;
    V.k = k;
    V.live = B.count;
    V.S = S;
    V.tiles_per_strip = ((int)((St.rows + GT_BN - 1) / GT_BN) + S - 1) / S;
    V.strip = (int)(blockIdx.x % (unsigned)S);
    V.perm = perm;
    V.valid = St.valid;
    V.xbits = reinterpret_cast<const uint32_t *>(excl_bits);
    V.W = W;
    rank_strip_walk<MODE, KL>(V, smem, ls, lr, llen);
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
    rank_finish_wave(live, good, live ? perm[p] : 0, lane, good && lane < S ? (p * S + lane) * k : -1, k, cand_s, cand_r,
                     tsc, trow, cnt, nullptr, topk_rows, topk_scores, rank, target_scores);
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

// The strip rule on the bound of the block count and the widest set's tiles.
static RmxPlan rmx_plan(int64_t Q, int64_t num_sets, int64_t max_rows, int64_t total_rows, int k) {
    RmxPlan p;
    p.max_blocks = Q / GT_BM + num_sets;
    int widest_tiles_per_strip;         // (a kernel derives its own set's)
    rank_strip_rule(p.max_blocks, (max_rows + GT_BN - 1) / GT_BN, p.S, widest_tiles_per_strip);
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
    rank_for_capacity(a.k, [&](auto kl) {
        hipLaunchKernelGGL((rmx_tile_kernel<MODE, decltype(kl)::value>), dim3((unsigned)(pl.max_blocks * pl.S)), dim3(256),
                           0, s, a.desc, a.blocks, a.state, a.perm, a.q, a.D, (const float *)a.rinv, (const float *)a.qinv,
                           (const float *)a.tsc, (const int *)a.trow, a.excl_bits, (long long)a.W, a.k, pl.S, a.cnt, a.cs,
                           a.cr);
    });
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
    rank_for_load_mode(ptr_vec_ok(q, dim), dim, [&](auto mode) { rmx_launch<decltype(mode)::value>(pl, a, s); });
    if (k > 0 || rank || target_scores)
        hipLaunchKernelGGL(rmx_finish_kernel, dim3((unsigned)((Q + 3) / 4)), dim3(256), 0, s, (long long)Q, k, pl.S,
                           (const RmxState *)state, (const int *)perm, (const float *)a.cs, (const int *)a.cr,
                           (const float *)a.tsc, (const int *)a.trow, (const int *)a.cnt, (long long *)topk_rows,
                           topk_scores, (long long *)rank, target_scores);
    return mpqe_launch_status();
}
