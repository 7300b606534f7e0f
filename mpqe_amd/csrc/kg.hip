// Answering a conjunctive query EXACTLY on the knowledge graph: which rows of the target mode's table reach every anchor
// along the formula's relations. Integer work only: one bitmap of a mode's rows per set (row r = bit r % 32 of word
// r / 32), one CSR per typed relation, OR along a hop, AND / OR across the branches, population counts.
//
// All seven query types are "1-3 branches, each a chain of 1-3 hops from one anchor; merge; then 0-1 hops" (the shape
// gqe.hip runs with matrices). One workgroup owns one query and walks the programme:
//   first hop of a branch   a list walk: the workgroup's 256 lanes stride over rows[offsets[a] .. offsets[a + 1])
//   a later hop             a scan of the frontier bitmap: the waves take its non-empty words in turn; for every set bit
//                           the wave's 64 lanes stride over that row's list (a row of degree 1 000 does not serialise on
//                           one lane)
//   merge                   AND (the answers) and OR (the union flavour the hard negatives come from) of the branches'
//                           bitmaps, word by word, in the same pass
//   hop after the merge     ONE scan of the OR bitmap: a set row's list goes to the union's result, and to the answers'
//                           result too if the row is in the AND bitmap (AND is a subset of OR)
//   out                     answers = the AND flavour; hard = the OR flavour & ~answers; counts = their population counts
//
// Home of the bitmaps. A workgroup keeps four: the ping-pong pair of a branch's hops and the two merge accumulators,
// each of W = ceil(n / 32) words for the widest mode the programme names. In LDS when W <= KG_LDS_WORDS = 2 432:
// 4 x 2 432 x 4 B = 38 912 B a workgroup, so four workgroups share a CU's 160 KiB (155 648 B + their 32 B of counters);
// that covers modes of up to 77 824 rows. Wider modes, and MPQE_KG_GLOBAL_BITS, keep the four bitmaps of query q at
// workspace[q * 4 * W ..] in HBM instead: the same code with atomicOr on global words, read back at agent scope (the OR
// is done in L2, so a plain load could meet a stale line of this CU's vector cache).
//
// Determinism: the only concurrent writes are integer ORs into a bitmap, whose result does not depend on their order;
// the output is a set, bit-identical run to run by construction. The workspace need not be zeroed: a bitmap is cleared
// by the workgroup right before it is ORed into, and every word of every output is written.
//
// Two kernels walk this programme: kg_answers_kernel (one formula a launch, the hops a KgPlan in kernel arguments) and
// kg_answers_mixed_kernel (the programme per QUERY, from its record; below). They share kg_or_list, kg_scan_hop and the
// bitmap helpers, and each still spells its own branch loop, merge, tail hop and write-out: a shared walk behind an
// accessor was measured 0.3 - 0.5 us slower on the AM shape's scanned hops and not kept. DESIGN.md section 10 lists what
// differs between the two; a change to one body belongs in the other.
#include <string.h>

#include <vector>

#include "common.h"
#include "kg_scan.h"
#include "kg_table.h"

#define KG_THREADS 256
#define KG_WAVES 4
#define KG_LDS_WORDS 2432
#define KG_MAX_ROWS ((int64_t)1 << 30)

struct KgHop {
    const long long *off;       // [n_src + 1]
    const long long *rows;      // [edges], rows of the destination mode
    long long edges;
    int n_src, n_dst;
};

struct KgPlan {
    int branches, tail, W, n_out, n_merge;
    int hops[3], anchor_n[3];
    KgHop hop[3][3];
    KgHop tail_hop;
};

__device__ __forceinline__ int kg_words(int n) { return (n + 31) >> 5; }

template <bool G>
__device__ __forceinline__ uint32_t kg_load(const uint32_t *p) {
    if (G) return agent_load(p);
    return *p;
}
template <bool G>
__device__ __forceinline__ void kg_store(uint32_t *p, uint32_t v) {
    if (G) agent_store(p, v); else *p = v;
}

template <bool G>
__device__ __forceinline__ void kg_clear(uint32_t *b, int n) {
    const int W = kg_words(n);
    for (int w = threadIdx.x; w < W; w += KG_THREADS) kg_store<G>(b + w, 0u);
}

// rows[offsets[x] .. offsets[x + 1]) ORed into `out` (and `out2`): entries id, id + stride, ... An offset outside
// [0, edges] or a row outside the destination mode is flagged and not followed.
__device__ __forceinline__ void kg_or_list(const KgHop &h, long long x, uint32_t *out, uint32_t *out2, int id, int stride,
                                           int32_t *err) {
    long long lo = h.off[x], hi = h.off[x + 1];
    if (lo < 0 || hi < lo || hi > h.edges) {
        flag_error(err, MPQE_FLAG_BAD_INDEX);
        lo = lo < 0 ? 0 : (lo > h.edges ? h.edges : lo);
        hi = hi < lo ? lo : (hi > h.edges ? h.edges : hi);
    }
    for (long long e = lo + id; e < hi; e += stride) {
        const long long r = h.rows[e];
        if (r < 0 || r >= h.n_dst) {
            flag_error(err, MPQE_FLAG_BAD_INDEX);
            continue;
        }
        const uint32_t bit = 1u << (unsigned)(r & 31);
        atomicOr(out + (r >> 5), bit);
        if (out2) atomicOr(out2 + (r >> 5), bit);
    }
}

// One hop from a frontier bitmap: every set row of `cur` sends its list to `out`; with `sub` (a subset of cur) a row
// that is in sub sends it to `out2` as well. Every wave reads the bitmap in chunks of 64 words, a lane per word, and ORs
// "my word is not zero" into a 64-bit mask over the wave: a chunk without a set bit -- nearly all of them on a large mode --
// costs one read and twelve shuffles. The non-empty words go to the four waves in turn (the k-th to wave k % 4); the
// owner takes the word from its lane and, for every set bit, its 64 lanes stride over that row's list. Every branch here
// is uniform in the wave.
template <bool G>
__device__ __forceinline__ void kg_scan_hop(const KgHop &h, const uint32_t *cur, const uint32_t *sub, uint32_t *out,
                                            uint32_t *out2, int32_t *err) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int Ws = kg_words(h.n_src);
    int k = 0;
    for (int c = 0; c < Ws; c += 64) {
        const int w = c + lane;
        const uint32_t mine = w < Ws ? kg_load<G>(cur + w) : 0u;
        const uint32_t mine_sub = sub && w < Ws ? kg_load<G>(sub + w) : 0u;
        int lo = mine && lane < 32 ? (int)(1u << lane) : 0, hi = mine && lane >= 32 ? (int)(1u << (lane - 32)) : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo |= __shfl_xor(lo, o, 64);
            hi |= __shfl_xor(hi, o, 64);
        }
        for (int half = 0; half < 2; ++half) {
            uint32_t words = (uint32_t)(half ? hi : lo);
            while (words) {
                const int j = __builtin_ctz(words) + 32 * half;
                words &= words - 1;
                if ((k++ & (KG_WAVES - 1)) != wave) continue;
                uint32_t bits = (uint32_t)__shfl((int)mine, j, 64);
                const uint32_t also = sub ? (uint32_t)__shfl((int)mine_sub, j, 64) : 0u;
                while (bits) {
                    const int b = __builtin_ctz(bits);
                    bits &= bits - 1;
                    const long long x = (long long)(c + j) * 32 + b;
                    if (x >= h.n_src) break;        // (never: bits at or above n are written as 0)
                    kg_or_list(h, x, out, ((also >> b) & 1u) ? out2 : nullptr, lane, 64, err);
                }
            }
        }
    }
}

template <bool G>
__global__ __launch_bounds__(KG_THREADS) void kg_answers_kernel(KgPlan P, const long long *__restrict__ anchors,
                                                                long long Q, uint32_t *__restrict__ answers,
                                                                uint32_t *__restrict__ hard,
                                                                long long *__restrict__ counts, uint32_t *ws,
                                                                int32_t *err) {
    __shared__ uint32_t lds[G ? 1 : 4 * KG_LDS_WORDS];
    __shared__ int red[2 * KG_WAVES];
    const long long q = blockIdx.x;
    const int t = threadIdx.x;
    uint32_t *base = G ? ws + (size_t)q * 4 * (size_t)P.W : lds;
    uint32_t *F[2] = {base, base + P.W};        // the ping-pong pair
    uint32_t *AND = base + 2 * (size_t)P.W, *OR = base + 3 * (size_t)P.W;
    const int Wout = kg_words(P.n_out);
    uint32_t *ans = answers + (size_t)q * Wout;
    uint32_t *hrd = hard ? hard + (size_t)q * Wout : nullptr;

    long long a[3] = {0, 0, 0};
    bool bad = false;
    for (int b = 0; b < P.branches; ++b) {
        a[b] = anchors[(long long)b * Q + q];
        bad = bad || a[b] < 0 || a[b] >= P.anchor_n[b];
    }
    if (bad) {          // (the whole workgroup: no barrier has been met yet) -- this query's sets are empty
        if (t == 0) flag_error(err, MPQE_FLAG_BAD_INDEX);
        for (int w = t; w < Wout; w += KG_THREADS) {
            ans[w] = 0u;
            if (hrd) hrd[w] = 0u;
        }
        if (counts && t == 0) {
            counts[q] = 0;
            counts[Q + q] = 0;
        }
        return;
    }

    for (int b = 0; b < P.branches; ++b) {
        const uint32_t *cur = nullptr;
        for (int s = 0; s < P.hops[b]; ++s) {
            const KgHop &h = P.hop[b][s];
            uint32_t *out = base + (size_t)(s & 1) * (size_t)P.W;
            kg_clear<G>(out, h.n_dst);
            __syncthreads();
            if (s == 0) kg_or_list(h, a[b], out, nullptr, t, KG_THREADS, err);
            else kg_scan_hop<G>(h, cur, nullptr, out, nullptr, err);
            __syncthreads();
            cur = out;
        }
        const int Wm = kg_words(P.n_merge);
        for (int w = t; w < Wm; w += KG_THREADS) {
            const uint32_t v = kg_load<G>(cur + w);
            if (b == 0) {
                kg_store<G>(AND + w, v);
                kg_store<G>(OR + w, v);
            } else {
                kg_store<G>(AND + w, kg_load<G>(AND + w) & v);
                kg_store<G>(OR + w, kg_load<G>(OR + w) | v);
            }
        }
        __syncthreads();
    }

    const uint32_t *res_and = AND, *res_or = OR;
    if (P.tail) {
        kg_clear<G>(F[0], P.tail_hop.n_dst);
        if (hrd) kg_clear<G>(F[1], P.tail_hop.n_dst);
        __syncthreads();
        if (hrd) kg_scan_hop<G>(P.tail_hop, OR, AND, F[1], F[0], err);
        else kg_scan_hop<G>(P.tail_hop, AND, nullptr, F[0], nullptr, err);
        __syncthreads();
        res_and = F[0];
        res_or = F[1];
    }

    int ca = 0, ch = 0;
    for (int w = t; w < Wout; w += KG_THREADS) {
        const uint32_t v = kg_load<G>(res_and + w);
        ans[w] = v;
        ca += __builtin_popcount(v);
        if (hrd) {
            const uint32_t u = kg_load<G>(res_or + w) & ~v;
            hrd[w] = u;
            ch += __builtin_popcount(u);
        }
    }
    if (!counts) return;        // (uniform)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ca += __shfl_xor(ca, o, 64);
        ch += __shfl_xor(ch, o, 64);
    }
    if ((t & 63) == 0) {
        red[t >> 6] = ca;
        red[KG_WAVES + (t >> 6)] = ch;
    }
    __syncthreads();
    if (t == 0) {
        counts[q] = (long long)red[0] + red[1] + red[2] + red[3];
        counts[Q + q] = (long long)red[4] + red[5] + red[6] + red[7];
    }
}

// ---------------------------------------------------------------------------------------------- bitmaps -> row lists
// One workgroup per query, 256 words a round: a lane counts its word, an exclusive scan over the workgroup places the
// word's rows, so a query's list comes out ascending. A slot outside [offsets[q], offsets[q + 1]) or past `cap` is not
// written and flagged, as is a list whose length is not what the offsets say.
__global__ __launch_bounds__(KG_THREADS) void kg_rows_kernel(const uint32_t *__restrict__ bits, long long n,
                                                             const uint32_t *__restrict__ valid, int select,
                                                             const long long *__restrict__ offsets,
                                                             long long *__restrict__ rows_out, long long cap,
                                                             int32_t *err) {
    __shared__ int wsum[KG_SCAN_WAVES];
    const long long q = blockIdx.x;
    const int t = threadIdx.x;
    const long long W = (n + 31) >> 5;
    const long long lo = offsets[q], hi = offsets[q + 1];
    if (lo < 0 || hi < lo || hi > cap) {        // (uniform)
        if (t == 0) flag_error(err, MPQE_FLAG_BAD_INDEX);
        return;
    }
    long long run = lo;
    bool over = false;
    for (long long w0 = 0; w0 < W; w0 += KG_THREADS) {
        const long long w = w0 + t;
        uint32_t v = 0u;
        if (w < W) {
            const uint32_t b = bits[q * W + w];
            const uint32_t va = valid ? valid[w] : ~0u;
            v = select == MPQE_KG_ROWS_SET ? b : (select == MPQE_KG_ROWS_COMPLEMENT ? va & ~b : b | ~va);
            if (w == W - 1 && (n & 31)) v &= (1u << (unsigned)(n & 31)) - 1u;
        }
        int total;
        long long p = run + kg_workgroup_scan(__builtin_popcount(v), wsum, total);
        while (v) {
            const int b = __builtin_ctz(v);
            v &= v - 1;
            if (p < hi) rows_out[p] = w * 32 + b; else over = true;
            ++p;
        }
        run += total;
        __syncthreads();        // (wsum is rewritten in the next round)
    }
    if (over || (t == 0 && run != hi)) flag_error(err, MPQE_FLAG_BAD_INDEX);
}

// ---------------------------------------------------------------------------------------------- host
static bool kg_mode_ok(int m, const int64_t *mode_rows, int num_modes) {
    return m >= 0 && m < num_modes && mode_rows[m] >= 1 && mode_rows[m] <= KG_MAX_ROWS;
}

// The programme checked and laid out; rel_* may be NULL (the size query: only modes are read). 0 = fine.
static int kg_compile(const int32_t *prog, const int64_t *const *rel_offsets, const int64_t *const *rel_rows,
                      const int64_t *rel_edges, int num_rels, const int64_t *mode_rows, int num_modes, KgPlan &P) {
    memset(&P, 0, sizeof(P));
    if (!prog || !mode_rows || num_modes < 1 || num_modes > 16) return MPQE_ERR_INVALID_ARG;
    const int branches = prog[1], tail = prog[5], target = prog[6];
    if (branches < 1 || branches > 3 || tail < 0 || tail > 1) return MPQE_ERR_INVALID_ARG;
    if (!kg_mode_ok(target, mode_rows, num_modes)) return MPQE_ERR_INVALID_ARG;
    int widest = 0, merge = -1;
    P.branches = branches;
    P.tail = tail;
    auto hop = [&](int code, int src_mode, KgHop &h, int &dst_mode) -> bool {
        if (code < 0) return false;
        const int rel = code >> 4;
        dst_mode = code & 15;
        if (!kg_mode_ok(dst_mode, mode_rows, num_modes)) return false;
        h.n_src = (int)mode_rows[src_mode];
        h.n_dst = (int)mode_rows[dst_mode];
        h.off = h.rows = nullptr;
        h.edges = 0;
        if (rel_offsets) {
            if (rel >= num_rels || !rel_offsets[rel] || rel_edges[rel] < 0) return false;
            if (rel_edges[rel] > 0 && !rel_rows[rel]) return false;
            h.off = reinterpret_cast<const long long *>(rel_offsets[rel]);
            h.rows = reinterpret_cast<const long long *>(rel_rows[rel]);
            h.edges = rel_edges[rel];
        }
        if (h.n_dst > widest) widest = h.n_dst;
        return true;
    };
    for (int b = 0; b < branches; ++b) {
        int mode = prog[8 + 5 * b];
        const int hops = prog[9 + 5 * b];
        if (!kg_mode_ok(mode, mode_rows, num_modes) || hops < 1 || hops > 3) return MPQE_ERR_INVALID_ARG;
        P.hops[b] = hops;
        P.anchor_n[b] = (int)mode_rows[mode];
        for (int s = 0; s < hops; ++s) {
            int dst;
            if (!hop(prog[10 + 5 * b + s], mode, P.hop[b][s], dst)) return MPQE_ERR_INVALID_ARG;
            mode = dst;
        }
        if (merge >= 0 && mode != merge) return MPQE_ERR_INVALID_ARG;       // the branches meet in ONE mode
        merge = mode;
    }
    P.n_merge = (int)mode_rows[merge];
    int last = merge;
    if (tail) {
        int dst;
        if (!hop(prog[24], merge, P.tail_hop, dst)) return MPQE_ERR_INVALID_ARG;
        last = dst;
    }
    if (last != target) return MPQE_ERR_INVALID_ARG;
    P.n_out = (int)mode_rows[target];
    P.W = (widest + 31) / 32;
    return MPQE_OK;
}

// The home of the bitmaps of W words each, what the workspace must hold for Q queries, and the launch: both answers entry
// points size, check and start their kernel here.
static bool kg_in_lds(int W, int flags) { return W <= KG_LDS_WORDS && !(flags & MPQE_KG_GLOBAL_BITS); }

static size_t kg_bitmap_bytes(int64_t Q, int W, int flags) {
    return kg_in_lds(W, flags) ? 256 : align_up((size_t)Q * 4 * (size_t)W * 4, 256) + 256;
}

// One workgroup a query of `lds_kernel` or `global_kernel`, the <false> and <true> of one kernel template, whose arguments
// are `args`, then the bitmaps' workspace (NULL in LDS) and the error word.
template <class... P, class... A>
static int kg_launch(void (*lds_kernel)(P...), void (*global_kernel)(P...), int64_t Q, int W, int flags, void *workspace,
                     size_t workspace_bytes, int32_t *err, void *stream, A... args) {
    const bool in_lds = kg_in_lds(W, flags);
    if (!in_lds && (!workspace || ((uintptr_t)workspace & 3))) return MPQE_ERR_INVALID_ARG;
    // (short of what the size query returns for these flags -- in LDS too, where the 256 bytes are not touched)
    if (workspace_bytes < kg_bitmap_bytes(Q, W, flags)) return MPQE_ERR_WORKSPACE;
    void (*kernel)(P...) = in_lds ? lds_kernel : global_kernel;
    hipLaunchKernelGGL(kernel, dim3((unsigned)Q), dim3(KG_THREADS), 0, as_stream(stream), args...,
                       in_lds ? nullptr : reinterpret_cast<uint32_t *>(workspace), err);
    return mpqe_launch_status();
}

extern "C" size_t mpqe_kg_workspace_bytes(const int32_t *prog_host, int64_t num_queries, const int64_t *mode_rows_host,
                                          int num_modes, int flags) {
    KgPlan P;
    if (num_queries < 0 || num_queries > KG_MAX_ROWS) return 0;
    if (kg_compile(prog_host, nullptr, nullptr, nullptr, 0, mode_rows_host, num_modes, P) != MPQE_OK) return 0;
    return kg_bitmap_bytes(num_queries, P.W, flags);
}

extern "C" int mpqe_kg_answers(const int32_t *prog_host, const int64_t *const *rel_offsets_host,
                               const int64_t *const *rel_rows_host, const int64_t *rel_edges_host, int num_rels,
                               const int64_t *mode_rows_host, int num_modes, const int64_t *anchor_rows,
                               int64_t num_queries, uint32_t *answers, uint32_t *hard, int64_t *counts, int flags,
                               void *workspace, size_t workspace_bytes, int32_t *err, void *stream) {
    const int64_t Q = num_queries;
    if (Q < 0 || Q > KG_MAX_ROWS || num_rels < 1 || !rel_offsets_host || !rel_rows_host || !rel_edges_host)
        return MPQE_ERR_INVALID_ARG;
    if (flags & ~MPQE_KG_GLOBAL_BITS) return MPQE_ERR_INVALID_ARG;
    KgPlan P;
    const int st = kg_compile(prog_host, rel_offsets_host, rel_rows_host, rel_edges_host, num_rels, mode_rows_host,
                              num_modes, P);
    if (st != MPQE_OK) return st;
    if (Q == 0) return MPQE_OK;
    if (!anchor_rows || !answers) return MPQE_ERR_INVALID_ARG;
    return kg_launch(kg_answers_kernel<false>, kg_answers_kernel<true>, Q, P.W, flags, workspace, workspace_bytes, err,
                     stream, P, reinterpret_cast<const long long *>(anchor_rows), (long long)Q, answers, hard,
                     reinterpret_cast<long long *>(counts));
}

extern "C" int mpqe_kg_rows(const uint32_t *bits, int64_t num_queries, int64_t n, const uint32_t *valid, int select,
                            const int64_t *offsets, int64_t *rows_out, int64_t rows_cap, int32_t *err, void *stream) {
    if (num_queries < 0 || num_queries > KG_MAX_ROWS || n < 1 || n > KG_MAX_ROWS || rows_cap < 0)
        return MPQE_ERR_INVALID_ARG;
    if (select != MPQE_KG_ROWS_SET && select != MPQE_KG_ROWS_COMPLEMENT && select != MPQE_KG_ROWS_WITH_HOLES)
        return MPQE_ERR_INVALID_ARG;
    if (num_queries == 0) return MPQE_OK;
    if (!bits || !offsets || (rows_cap > 0 && !rows_out)) return MPQE_ERR_INVALID_ARG;
    hipLaunchKernelGGL(kg_rows_kernel, dim3((unsigned)num_queries), dim3(KG_THREADS), 0, as_stream(stream), bits,
                       (long long)n, valid, select, reinterpret_cast<const long long *>(offsets),
                       reinterpret_cast<long long *>(rows_out), (long long)rows_cap, err);
    return mpqe_launch_status();
}

// ------------------------------------------------------------------------- queries of DIFFERENT formulas, one launch
// mpqe_kg_answers_mixed: the kernel above with the programme taken per QUERY. The launch fixes the query type -- the hop
// structure, KgShape, in the hop order of kg.query_hops -- and every workgroup reads its relations from its own record
// (the layout mpqe_kg_sample_queries writes) and follows them through the index's device table (kg_table.h): the hop of
// query edge (x, rel, y) walks the CSR of table[rel].reverse. Thread 0 resolves and checks the record into LDS; the walk is
// the one above (kg_or_list, kg_scan_hop, both homes of the bitmaps, W = the widest mode of the index).
// CSR faults are collected in an LDS word of the workgroup, not in the caller's: a query that met one gets empty sets like
// any other malformed query, and the caller's word takes one atomic a faulty workgroup instead of one a faulty entry.
struct KgShape {
    int branches, tail_edge;    // tail_edge: the query edge of the hop after the merge, -1: none
    int hops[3];
    int edge[3][3];             // [b][s]: the query edge whose reverse relation hop s of branch b walks
};

enum { KGM_OK = 0, KGM_NONE = 1, KGM_BAD = 2 };

struct KgMixedQuery {
    KgHop hop[3];               // per query EDGE: the CSR of the edge's reverse relation
    int src[3], dst[3];         // its modes
    long long anchor[3];        // per branch
    long long probe;
    int state, n_merge, n_out, target;
};

__device__ __forceinline__ void kg_mixed_resolve(const KgShape &S, const char *table, int W, const long long *rec,
                                                 const long long *probe_rows, long long q, KgMixedQuery &M) {
    const KgtHead &H = *kgt_head(table);
    const KgtRel *rel = kgt_rels(table);
    M.state = KGM_BAD;
    M.n_merge = M.n_out = 0;
    M.target = -1;
    M.probe = -1;
    if (rec[0] == 0) {
        M.state = KGM_NONE;
        return;
    }
    if (rec[0] != 1 || H.magic != KGT_MAGIC || H.num_rels < 1 || H.num_rels > KGT_MAX_RELS) return;
    unsigned used = 0u;         // a bit per query edge
    for (int b = 0; b < S.branches; ++b)
        for (int s = 0; s < S.hops[b]; ++s) used |= 1u << S.edge[b][s];
    if (S.tail_edge >= 0) used |= 1u << S.tail_edge;
    for (int e = 0; e < 3; ++e) {
        if (!((used >> e) & 1u)) continue;
        const long long r = rec[2 + 3 * e];
        if (r < 0 || r >= H.num_rels) return;
        const int rv = rel[r].reverse;
        if (rv < 0 || rv >= H.num_rels) return;
        const KgtRel &R = rel[rv];
        // (a table of another index than the host's mode_rows: its bitmaps would not fit the W words of this launch)
        if (R.n_src < 1 || R.n_dst < 1 || kg_words(R.n_src) > W || kg_words(R.n_dst) > W || R.edges < 0) return;
        M.hop[e].off = R.off;
        M.hop[e].rows = R.rows;
        M.hop[e].edges = R.edges;
        M.hop[e].n_src = R.n_src;
        M.hop[e].n_dst = R.n_dst;
        M.src[e] = R.src;
        M.dst[e] = R.dst;
    }
    int merge = -1;
    for (int b = 0; b < S.branches; ++b) {
        const int first = S.edge[b][0];
        int mode = M.src[first];
        const long long a = rec[3 + 3 * first];         // the leaf edge's destination row
        if (a < 0 || a >= M.hop[first].n_src) return;
        M.anchor[b] = a;
        for (int s = 0; s < S.hops[b]; ++s) {
            const int e = S.edge[b][s];
            if (M.src[e] != mode) return;
            mode = M.dst[e];
        }
        if (merge >= 0 && mode != merge) return;
        merge = mode;
    }
    int last = merge;
    if (S.tail_edge >= 0) {
        if (M.src[S.tail_edge] != merge) return;
        last = M.dst[S.tail_edge];
    }
    if (merge < 0 || merge >= H.num_modes || last < 0 || last >= H.num_modes) return;
    M.n_merge = (int)H.mode_rows[merge];
    M.n_out = (int)H.mode_rows[last];
    if (kg_words(M.n_merge) > W || kg_words(M.n_out) > W) return;
    M.target = last;
    M.probe = probe_rows ? probe_rows[q] : rec[1];
    M.state = KGM_OK;
}

template <bool G>
__global__ __launch_bounds__(KG_THREADS) void kg_answers_mixed_kernel(
    KgShape S, const char *__restrict__ table, int W, bool want_hard, const long long *__restrict__ records,
    const long long *__restrict__ probe_rows, long long Q, uint32_t *__restrict__ answers, uint32_t *__restrict__ hard,
    long long out_words, long long *__restrict__ counts, int32_t *__restrict__ target_mode, int32_t *__restrict__ member,
    uint32_t *ws, int32_t *err) {
    __shared__ uint32_t lds[G ? 1 : 4 * KG_LDS_WORDS];
    __shared__ int red[2 * KG_WAVES];
    __shared__ KgMixedQuery M;
    __shared__ int32_t wg_err;
    const long long q = blockIdx.x;
    const int t = threadIdx.x;
    if (t == 0) {
        wg_err = 0;
        kg_mixed_resolve(S, table, W, records + q * MPQE_KG_QUERY_INTS, probe_rows, q, M);
    }
    __syncthreads();
    uint32_t *ans = answers ? answers + (size_t)q * (size_t)out_words : nullptr;
    uint32_t *hrd = hard ? hard + (size_t)q * (size_t)out_words : nullptr;
    bool empty = M.state != KGM_OK;             // (uniform)
    const uint32_t *res_and = nullptr, *res_or = nullptr;
    if (!empty) {
        uint32_t *base = G ? ws + (size_t)q * 4 * (size_t)W : lds;
        uint32_t *F[2] = {base, base + W};
        uint32_t *AND = base + 2 * (size_t)W, *OR = base + 3 * (size_t)W;
        for (int b = 0; b < S.branches; ++b) {
            const uint32_t *cur = nullptr;
            for (int s = 0; s < S.hops[b]; ++s) {
                const KgHop &h = M.hop[S.edge[b][s]];
                uint32_t *out = F[s & 1];
                kg_clear<G>(out, h.n_dst);
                __syncthreads();
                if (s == 0) kg_or_list(h, M.anchor[b], out, nullptr, t, KG_THREADS, &wg_err);
                else kg_scan_hop<G>(h, cur, nullptr, out, nullptr, &wg_err);
                __syncthreads();
                cur = out;
            }
            const int Wm = kg_words(M.n_merge);
            for (int w = t; w < Wm; w += KG_THREADS) {
                const uint32_t v = kg_load<G>(cur + w);
                if (b == 0) {
                    kg_store<G>(AND + w, v);
                    kg_store<G>(OR + w, v);
                } else {
                    kg_store<G>(AND + w, kg_load<G>(AND + w) & v);
                    kg_store<G>(OR + w, kg_load<G>(OR + w) | v);
                }
            }
            __syncthreads();
        }
        res_and = AND;
        res_or = OR;
        if (S.tail_edge >= 0) {
            const KgHop &h = M.hop[S.tail_edge];
            kg_clear<G>(F[0], h.n_dst);
            if (want_hard) kg_clear<G>(F[1], h.n_dst);
            __syncthreads();
            if (want_hard) kg_scan_hop<G>(h, OR, AND, F[1], F[0], &wg_err);
            else kg_scan_hop<G>(h, AND, nullptr, F[0], nullptr, &wg_err);
            __syncthreads();
            res_and = F[0];
            res_or = F[1];
        }
        empty = wg_err != 0;                    // (every OR into it lies before a barrier met above)
    }
    if (empty) {
        for (long long w = t; w < out_words; w += KG_THREADS) {
            if (ans) ans[w] = 0u;
            if (hrd) hrd[w] = 0u;
        }
        if (t == 0) {
            if (M.state != KGM_NONE) flag_error(err, MPQE_FLAG_BAD_INDEX);
            if (counts) {
                counts[q] = 0;
                counts[Q + q] = 0;
            }
            target_mode[q] = -1;
            if (member) member[q] = 0;
        }
        return;
    }
    const int Wout = kg_words(M.n_out);
    int ca = 0, ch = 0;
    for (int w = t; w < Wout; w += KG_THREADS) {
        const uint32_t v = kg_load<G>(res_and + w);
        if (ans) ans[w] = v;
        ca += __builtin_popcount(v);
        if (want_hard) {
            const uint32_t u = kg_load<G>(res_or + w) & ~v;
            if (hrd) hrd[w] = u;
            ch += __builtin_popcount(u);
        }
    }
    for (long long w = Wout + t; w < out_words; w += KG_THREADS) {
        if (ans) ans[w] = 0u;
        if (hrd) hrd[w] = 0u;
    }
    if (t == 0) {
        target_mode[q] = M.target;
        if (member) {
            const long long p = M.probe;
            member[q] = p >= 0 && p < M.n_out ? (int)((kg_load<G>(res_and + (p >> 5)) >> (unsigned)(p & 31)) & 1u) : 0;
        }
    }
    if (!counts) return;        // (uniform)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ca += __shfl_xor(ca, o, 64);
        ch += __shfl_xor(ch, o, 64);
    }
    if ((t & 63) == 0) {
        red[t >> 6] = ca;
        red[KG_WAVES + (t >> 6)] = ch;
    }
    __syncthreads();
    if (t == 0) {
        counts[q] = (long long)red[0] + red[1] + red[2] + red[3];
        counts[Q + q] = (long long)red[4] + red[5] + red[6] + red[7];
    }
}

// the hop structure of a query type: kg.query_hops in query EDGES (mpqe_kg_sample_queries' edge order)
static bool kg_shape(int qt, KgShape &S) {
    memset(&S, 0, sizeof(S));
    S.tail_edge = -1;
    auto branch = [&](int e0, int e1, int e2) {
        const int b = S.branches++;
        S.edge[b][0] = e0;
        S.edge[b][1] = e1 < 0 ? 0 : e1;
        S.edge[b][2] = e2 < 0 ? 0 : e2;
        S.hops[b] = 1 + (e1 >= 0) + (e2 >= 0);
    };
    switch (qt) {
    case MPQE_Q_1CHAIN: branch(0, -1, -1); return true;
    case MPQE_Q_2CHAIN: branch(1, 0, -1); return true;
    case MPQE_Q_3CHAIN: branch(2, 1, 0); return true;
    case MPQE_Q_2INTER: branch(0, -1, -1); branch(1, -1, -1); return true;
    case MPQE_Q_3INTER: branch(0, -1, -1); branch(1, -1, -1); branch(2, -1, -1); return true;
    case MPQE_Q_3INTER_CHAIN: branch(0, -1, -1); branch(2, 1, -1); return true;
    case MPQE_Q_3CHAIN_INTER: branch(1, -1, -1); branch(2, -1, -1); S.tail_edge = 0; return true;
    default: return false;
    }
}

// the widest mode's words; 0: arguments out of range
static int kg_mixed_words(const int64_t *mode_rows, int num_modes) {
    const int64_t widest = kgt_widest_mode(mode_rows, num_modes);
    return widest > KG_MAX_ROWS ? 0 : (int)((widest + 31) / 32);
}

extern "C" size_t mpqe_kg_mixed_workspace_bytes(int64_t num_queries, const int64_t *mode_rows_host, int num_modes,
                                                int flags) {
    const int W = kg_mixed_words(mode_rows_host, num_modes);
    if (W == 0 || num_queries < 0 || num_queries > KG_MAX_ROWS) return 0;
    return kg_bitmap_bytes(num_queries, W, flags);
}

extern "C" size_t mpqe_kg_table_bytes(int num_rels, int num_modes) {
    if (num_rels < 1 || num_rels > KGT_MAX_RELS || num_modes < 1 || num_modes > KGT_MAX_MODES) return 0;
    return align_up(sizeof(KgtHead) + (size_t)num_rels * sizeof(KgtRel), 256);
}

extern "C" int mpqe_kg_table_build(const int64_t *const *rel_offsets_host, const int64_t *const *rel_rows_host,
                                   const int64_t *rel_edges_host, const int32_t *rel_src_mode_host,
                                   const int32_t *rel_dst_mode_host, const int32_t *rel_reverse_host, int num_rels,
                                   const int64_t *mode_rows_host, const uint32_t *const *mode_valid_host,
                                   const int64_t *const *mode_row_ids_host, int num_modes, void *table, size_t table_bytes,
                                   void *stream) {
    const size_t need = mpqe_kg_table_bytes(num_rels, num_modes);
    if (need == 0 || !rel_offsets_host || !rel_rows_host || !rel_edges_host || !rel_src_mode_host || !rel_dst_mode_host ||
        !rel_reverse_host || kg_mixed_words(mode_rows_host, num_modes) == 0)
        return MPQE_ERR_INVALID_ARG;
    if (!table || ((uintptr_t)table & 7)) return MPQE_ERR_INVALID_ARG;
    if (table_bytes < need) return MPQE_ERR_WORKSPACE;
    static thread_local std::vector<char> store;       // (outlives the copy below, as mpqe_kg_sample_queries' does)
    store.assign(need, 0);
    char *image = store.data();
    KgtHead *H = reinterpret_cast<KgtHead *>(image);
    KgtRel *R = reinterpret_cast<KgtRel *>(image + sizeof(KgtHead));
    H->num_rels = num_rels;
    H->num_modes = num_modes;
    H->magic = KGT_MAGIC;
    for (int m = 0; m < num_modes; ++m) {
        H->mode_rows[m] = mode_rows_host[m];
        H->valid[m] = mode_valid_host ? mode_valid_host[m] : nullptr;
        H->row_ids[m] = mode_row_ids_host ? reinterpret_cast<const long long *>(mode_row_ids_host[m]) : nullptr;
    }
    for (int i = 0; i < num_rels; ++i) {
        const int src = rel_src_mode_host[i], dst = rel_dst_mode_host[i], rv = rel_reverse_host[i];
        if (src < 0 || src >= num_modes || dst < 0 || dst >= num_modes || rv < -1 || rv >= num_rels) return MPQE_ERR_INVALID_ARG;
        if (!rel_offsets_host[i] || rel_edges_host[i] < 0 || (rel_edges_host[i] > 0 && !rel_rows_host[i]))
            return MPQE_ERR_INVALID_ARG;
        R[i].off = reinterpret_cast<const long long *>(rel_offsets_host[i]);
        R[i].rows = reinterpret_cast<const long long *>(rel_rows_host[i]);
        R[i].edges = rel_edges_host[i];
        R[i].n_src = (int)mode_rows_host[src];
        R[i].n_dst = (int)mode_rows_host[dst];
        R[i].src = src;
        R[i].dst = dst;
        R[i].reverse = rv;
    }
    hipStream_t s = as_stream(stream);
    if (hipMemcpyAsync(table, image, need, hipMemcpyHostToDevice, s) != hipSuccess) return MPQE_ERR_LAUNCH;
    return MPQE_OK;
}

extern "C" int mpqe_kg_answers_mixed(const void *table, const int64_t *mode_rows_host, int num_modes, int query_type,
                                     const int64_t *records, int64_t num_queries, const int64_t *probe_rows,
                                     uint32_t *answers, uint32_t *hard, int64_t out_words, int64_t *counts,
                                     int32_t *target_mode, int32_t *member, int flags, void *workspace,
                                     size_t workspace_bytes, int32_t *err, void *stream) {
    const int64_t Q = num_queries;
    const int W = kg_mixed_words(mode_rows_host, num_modes);
    KgShape S;
    if (W == 0 || Q < 0 || Q > KG_MAX_ROWS || !kg_shape(query_type, S)) return MPQE_ERR_INVALID_ARG;
    if (flags & ~(MPQE_KG_GLOBAL_BITS | MPQE_KG_COUNT_HARD)) return MPQE_ERR_INVALID_ARG;
    if ((answers || hard) && out_words < W) return MPQE_ERR_INVALID_ARG;
    if (Q == 0) return MPQE_OK;
    if (!table || ((uintptr_t)table & 7) || !records || !target_mode) return MPQE_ERR_INVALID_ARG;
    const bool want_hard = hard != nullptr || (flags & MPQE_KG_COUNT_HARD);
    const long long words = answers || hard ? (long long)out_words : 0;
    return kg_launch(kg_answers_mixed_kernel<false>, kg_answers_mixed_kernel<true>, Q, W, flags, workspace, workspace_bytes,
                     err, stream, S, reinterpret_cast<const char *>(table), W, want_hard,
                     reinterpret_cast<const long long *>(records), reinterpret_cast<const long long *>(probe_rows),
                     (long long)Q, answers, hard, words, reinterpret_cast<long long *>(counts), target_mode, member);
}
