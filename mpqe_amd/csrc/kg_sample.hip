// Sampling on the knowledge-graph index: grounded queries by the reference's random walk, and a bounded number of members
// of a query's answer / negative set. Integer work only, no float and no float atomics. The conventions are kg.hip's:
// every set, id and offset is in TABLE ROWS of a mode; the host passes arrays of device pointers; a CSR offset or row is
// clamped / checked and flagged (MPQE_FLAG_BAD_INDEX), never trusted; arguments are checked before any launch.
//
// The random stream (include/mpqe_amd.h spells it out; tests/kg_sample_oracle.py restates it with Python ints) is the
// library's counter-based one: mpqe_mix64 (splitmix64's finaliser) over (seed, slot, try, draw number), reduced with
// `% length` as mpqe_sample_negatives does. No state: a slot's record is a pure function of the seed and the graph.
//
// mpqe_kg_sample_queries  Graph.sample_query_subgraph_bytype (reference graph.py:321-389). One lane per slot in
//   256-thread workgroups: a walk is 3-8 dependent loads a try and diverges by construction, so it is latency bound and
//   there is nothing to share between lanes. The per-relation table (~100 typed relations on an AIFB-like schema) does not
//   fit kernel arguments; the host lays it out in the caller's workspace.
//   The "flat adjacency" of a row x of mode m is the concatenation, in relation-index order, of x's lists in every
//   relation whose source mode is m; a draw is uniform over its entries (so a relation is met in proportion to x's degree
//   in it, NOT uniformly). Edges out of one node are redrawn until their (relation, neighbour) pairs differ; the index
//   allows repeated CSR entries, so a redraw loop gives up after KGS_MAX_REDRAWS draws and the try is rejected.
//
// mpqe_kg_sample_rows  at most k members of every query's selected set. One workgroup per query: population counts of
//   the selected words summed per chunk of 64 words, an exclusive scan of the chunk sums in LDS; the member of rank r is
//   then a binary search over the chunk sums, a walk over the chunk's words and a select inside the word. With c <= k
//   members the ranks are 0 .. c - 1 (the list of mpqe_kg_rows, bit for bit); with more, rank j = P(j), j < k, for a keyed
//   bijection P of [0, c): a KGS_FEISTEL_ROUNDS-round balanced Feistel network over [0, 4^h), 4^h >= c, walked along its
//   cycle until it lands below c. No memory, no sort; distinct by construction.
//
// mpqe_kg_sample_rows_mixed  the same draw (kgs_chunk_sums, kgs_member, kgs_draw: ONE copy) for queries of different modes:
//   n and valid per query from the index's device table (kg_table.h), a row stride for `bits`, q_base in the draw key, and
//   the lists as entity ids too.
#include <string.h>

#include <vector>

#include "kg_scan.h"
#include "kg_stream.h"
#include "kg_table.h"

#define KGS_THREADS 256
#define KGS_WAVES 4
#define KGS_MAX_REDRAWS 64
#define KGS_MAX_RELS 4096
#define KGS_MAX_MODES 16
#define KGS_MAX_TRIES 1024
#define KGS_MAX_SLOTS ((int64_t)1 << 30)
#define KGS_REC_INTS MPQE_KG_QUERY_INTS
#define KGS_MAX_K MPQE_KG_SAMPLE_MAX_K
#define KGS_MAX_SAMPLE_ROWS MPQE_KG_SAMPLE_MAX_ROWS
#define KGS_CHUNK_WORDS 64
#define KGS_MAX_CHUNKS (KGS_MAX_SAMPLE_ROWS / 32 / KGS_CHUNK_WORDS)      // 2 048

// ------------------------------------------------------------------------------------------------------ the walk
struct KgsRel {
    const long long *off;       // [rows(src) + 1]
    const long long *rows;      // [edges], rows of the destination mode
    const long long *start;     // [n_start]: the source rows with a non-empty list
    long long edges, n_start;
    int src, dst, pad[2];
};

struct KgsHead {
    long long mode_rows[KGS_MAX_MODES];
    int mode_begin[KGS_MAX_MODES + 1];      // mode m's relations: mode_rels[mode_begin[m] .. mode_begin[m + 1])
    int num_rels, num_modes, n_active, pad;
};
// workspace: KgsHead | KgsRel [num_rels] | int active [num_rels] | int mode_rels [num_rels]

struct KgsTable {
    const KgsHead *head;
    const KgsRel *rel;
    const int *active, *mode_rels;
};

struct KgsDraws {
    unsigned long long key;
    unsigned d;
    __device__ __forceinline__ long long next(long long len) {
        return (long long)(mpqe_mix64(key ^ (unsigned long long)(d++)) % (unsigned long long)len);
    }
};

// x's list in relation r, clamped: false (and flagged) if the offsets are outside [0, edges] or out of order
__device__ __forceinline__ bool kgs_list(const KgsRel &r, long long x, long long &lo, long long &hi, int32_t *err) {
    lo = r.off[x];
    hi = r.off[x + 1];
    if (lo < 0 || hi < lo || hi > r.edges) {
        flag_error(err, MPQE_FLAG_BAD_INDEX);
        return false;
    }
    return true;
}

// entries of the flat adjacency of row x of `mode`; -1: a corrupt offset (flagged)
__device__ __forceinline__ long long kgs_flat_degree(const KgsTable &T, int mode, long long x, int32_t *err) {
    long long total = 0;
    for (int i = T.head->mode_begin[mode]; i < T.head->mode_begin[mode + 1]; ++i) {
        long long lo, hi;
        if (!kgs_list(T.rel[T.mode_rels[i]], x, lo, hi, err)) return -1;
        total += hi - lo;
    }
    return total;
}

// entry j (< the flat degree) of the flat adjacency -> (relation, neighbour); false: a neighbour outside its mode (flagged)
__device__ __forceinline__ bool kgs_flat_entry(const KgsTable &T, int mode, long long x, long long j, int &rel,
                                               long long &y, int32_t *err) {
    for (int i = T.head->mode_begin[mode]; i < T.head->mode_begin[mode + 1]; ++i) {
        const int ri = T.mode_rels[i];
        const KgsRel &r = T.rel[ri];
        long long lo, hi;
        if (!kgs_list(r, x, lo, hi, err)) return false;
        if (j < hi - lo) {
            y = r.rows[lo + j];
            rel = ri;
            if (y < 0 || y >= T.head->mode_rows[r.dst]) {
                flag_error(err, MPQE_FLAG_BAD_INDEX);
                return false;
            }
            return true;
        }
        j -= hi - lo;
    }
    return false;           // (never: j is below the degree the same offsets gave)
}

// One try of slot's walk into e[9] = three (source row, relation, destination row); false = rejected.
__device__ bool kgs_try(const KgsTable &T, int qt, KgsDraws &D, long long *e, int32_t *err) {
    const KgsHead &H = *T.head;
    if (H.n_active < 1) return false;
    const KgsRel &r0 = T.rel[T.active[D.next(H.n_active)]];
    const long long x = r0.start[D.next(r0.n_start)];
    const int mode = r0.src;
    if (x < 0 || x >= H.mode_rows[mode]) {
        flag_error(err, MPQE_FLAG_BAD_INDEX);
        return false;
    }
    // `fan` edges out of node `at` of mode `m` into e[3 * first ..], pairwise different in (relation, neighbour)
    auto edges_out = [&](long long at, int m, int fan, int first) -> bool {
        const long long deg = kgs_flat_degree(T, m, at, err);
        if (deg < fan) return false;        // (the reference's `num_edges > len(flat_adj_lists)`; -1: corrupt)
        for (int i = 0; i < fan; ++i) {
            int rel = -1;
            long long y = -1;
            int redraws = 0;
            for (;;) {
                if (!kgs_flat_entry(T, m, at, D.next(deg), rel, y, err)) return false;
                bool same = false;
                for (int p = 0; p < i; ++p) same = same || (e[3 * (first + p) + 1] == rel && e[3 * (first + p) + 2] == y);
                if (!same) break;
                if (++redraws >= KGS_MAX_REDRAWS) return false;     // repeated CSR entries: give up, never spin
            }
            e[3 * (first + i)] = at;
            e[3 * (first + i) + 1] = rel;
            e[3 * (first + i) + 2] = y;
        }
        return true;
    };
    auto dst_mode = [&](int edge) { return T.rel[e[3 * edge + 1]].dst; };
    switch (qt) {
    case MPQE_Q_1CHAIN:
        return edges_out(x, mode, 1, 0);
    case MPQE_Q_2CHAIN:
        return edges_out(x, mode, 1, 0) && edges_out(e[2], dst_mode(0), 1, 1);
    case MPQE_Q_3CHAIN:
        return edges_out(x, mode, 1, 0) && edges_out(e[2], dst_mode(0), 1, 1) && edges_out(e[5], dst_mode(1), 1, 2);
    case MPQE_Q_2INTER:
        return edges_out(x, mode, 2, 0);
    case MPQE_Q_3INTER:
        return edges_out(x, mode, 3, 0);
    case MPQE_Q_3INTER_CHAIN:
        return edges_out(x, mode, 2, 0) && edges_out(e[5], dst_mode(1), 1, 2);
    default:            // MPQE_Q_3CHAIN_INTER
        return edges_out(x, mode, 1, 0) && edges_out(e[2], dst_mode(0), 2, 1);
    }
}

__host__ __device__ __forceinline__ int kgs_type_edges(int qt) {
    return qt == MPQE_Q_1CHAIN ? 1 : (qt == MPQE_Q_2CHAIN || qt == MPQE_Q_2INTER ? 2 : 3);
}

__global__ __launch_bounds__(KGS_THREADS) void kg_sample_queries_kernel(const char *__restrict__ ws, int qt, long long Q,
                                                                        int max_tries, unsigned long long seed,
                                                                        long long *__restrict__ out, int32_t *err) {
    const long long q = (long long)blockIdx.x * KGS_THREADS + threadIdx.x;
    if (q >= Q) return;
    KgsTable T;
    T.head = reinterpret_cast<const KgsHead *>(ws);
    T.rel = reinterpret_cast<const KgsRel *>(ws + sizeof(KgsHead));
    T.active = reinterpret_cast<const int *>(ws + sizeof(KgsHead) + (size_t)T.head->num_rels * sizeof(KgsRel));
    T.mode_rels = T.active + T.head->num_rels;
    const int edges = kgs_type_edges(qt);
    const unsigned long long base = mpqe_mix64(seed ^ mpqe_mix64((unsigned long long)q));
    long long e[9];
    bool found = false;
    for (int t = 0; t < max_tries && !found; ++t) {
        KgsDraws D = {mpqe_mix64(base ^ (unsigned long long)t), 0u};
        found = kgs_try(T, qt, D, e, err);
    }
    long long *rec = out + q * KGS_REC_INTS;
    rec[0] = found ? 1 : 0;
    for (int i = 0; i < 9; ++i) rec[1 + i] = found && i < 3 * edges ? e[i] : -1;
}

static size_t kgs_ws_bytes(int num_rels) {
    return align_up(sizeof(KgsHead) + (size_t)num_rels * (sizeof(KgsRel) + 2 * sizeof(int)), 256);
}

extern "C" size_t mpqe_kg_sample_workspace_bytes(int num_rels, int num_modes) {
    if (num_rels < 1 || num_rels > KGS_MAX_RELS || num_modes < 1 || num_modes > KGS_MAX_MODES) return 0;
    return kgs_ws_bytes(num_rels);
}

extern "C" int mpqe_kg_sample_queries(const int64_t *const *rel_offsets_host, const int64_t *const *rel_rows_host,
                                      const int64_t *rel_edges_host, const int32_t *rel_src_mode_host,
                                      const int32_t *rel_dst_mode_host, const int64_t *const *rel_start_rows_host,
                                      const int64_t *rel_start_count_host, int num_rels, const int64_t *mode_rows_host,
                                      int num_modes, int query_type, int64_t num_slots, int max_tries, uint64_t seed,
                                      int64_t *out, void *workspace, size_t workspace_bytes, int32_t *err, void *stream) {
    if (num_rels < 1 || num_rels > KGS_MAX_RELS || num_modes < 1 || num_modes > KGS_MAX_MODES) return MPQE_ERR_INVALID_ARG;
    if (!rel_offsets_host || !rel_rows_host || !rel_edges_host || !rel_src_mode_host || !rel_dst_mode_host ||
        !rel_start_rows_host || !rel_start_count_host || !mode_rows_host)
        return MPQE_ERR_INVALID_ARG;
    if (query_type < 0 || query_type >= MPQE_Q_COUNT || num_slots < 0 || num_slots > KGS_MAX_SLOTS) return MPQE_ERR_INVALID_ARG;
    if (max_tries < 1 || max_tries > KGS_MAX_TRIES) return MPQE_ERR_INVALID_ARG;
    for (int m = 0; m < num_modes; ++m)
        if (mode_rows_host[m] < 1 || mode_rows_host[m] > ((int64_t)1 << 30)) return MPQE_ERR_INVALID_ARG;
    static thread_local std::vector<char> image;       // (outlives the copy below)
    image.assign(kgs_ws_bytes(num_rels), 0);
    KgsHead *H = reinterpret_cast<KgsHead *>(image.data());
    KgsRel *R = reinterpret_cast<KgsRel *>(image.data() + sizeof(KgsHead));
    int *active = reinterpret_cast<int *>(image.data() + sizeof(KgsHead) + (size_t)num_rels * sizeof(KgsRel));
    int *mode_rels = active + num_rels;
    H->num_rels = num_rels;
    H->num_modes = num_modes;
    for (int m = 0; m < num_modes; ++m) H->mode_rows[m] = mode_rows_host[m];
    for (int i = 0; i < num_rels; ++i) {
        const int src = rel_src_mode_host[i], dst = rel_dst_mode_host[i];
        const int64_t edges = rel_edges_host[i], starts = rel_start_count_host[i];
        if (src < 0 || src >= num_modes || dst < 0 || dst >= num_modes || !rel_offsets_host[i] || edges < 0)
            return MPQE_ERR_INVALID_ARG;
        if (edges > 0 && !rel_rows_host[i]) return MPQE_ERR_INVALID_ARG;
        if (starts < 0 || starts > mode_rows_host[src] || starts > edges) return MPQE_ERR_INVALID_ARG;
        if (starts > 0 && !rel_start_rows_host[i]) return MPQE_ERR_INVALID_ARG;
        R[i].off = reinterpret_cast<const long long *>(rel_offsets_host[i]);
        R[i].rows = reinterpret_cast<const long long *>(rel_rows_host[i]);
        R[i].start = reinterpret_cast<const long long *>(rel_start_rows_host[i]);
        R[i].edges = edges;
        R[i].n_start = starts;
        R[i].src = src;
        R[i].dst = dst;
        if (starts > 0) active[H->n_active++] = i;      // a relation without an edge is never the start
    }
    int at = 0;
    for (int m = 0; m < num_modes; ++m) {
        H->mode_begin[m] = at;
        for (int i = 0; i < num_rels; ++i)
            if (rel_src_mode_host[i] == m) mode_rels[at++] = i;
    }
    for (int m = num_modes; m <= KGS_MAX_MODES; ++m) H->mode_begin[m] = at;
    if (num_slots == 0) return MPQE_OK;
    if (!out || !workspace || ((uintptr_t)workspace & 7)) return MPQE_ERR_INVALID_ARG;
    if (workspace_bytes < image.size()) return MPQE_ERR_WORKSPACE;
    hipStream_t s = as_stream(stream);
    if (hipMemcpyAsync(workspace, image.data(), image.size(), hipMemcpyHostToDevice, s) != hipSuccess) return MPQE_ERR_LAUNCH;
    hipLaunchKernelGGL(kg_sample_queries_kernel, dim3((unsigned)((num_slots + KGS_THREADS - 1) / KGS_THREADS)),
                       dim3(KGS_THREADS), 0, s, reinterpret_cast<const char *>(workspace), query_type, (long long)num_slots,
                       max_tries, (unsigned long long)seed, reinterpret_cast<long long *>(out), err);
    return mpqe_launch_status();
}

// ------------------------------------------------------------------------------------ at most k members of a set
// One query's selected set: the rows below n whose bit in `bits` is set (MPQE_KG_ROWS_SET), or is not and whose bit in
// `valid` is (MPQE_KG_ROWS_COMPLEMENT; valid NULL: every row below n).
struct KgsSet {
    const uint32_t *bits, *valid;
    int select;
    long long n, W;
    int chunks;                 // of KGS_CHUNK_WORDS words
    __device__ __forceinline__ KgsSet(const uint32_t *bits_, const uint32_t *valid_, int select_, long long n_)
        : bits(bits_), valid(valid_), select(select_), n(n_), W((n_ + 31) >> 5),
          chunks((int)((W + KGS_CHUNK_WORDS - 1) / KGS_CHUNK_WORDS)) {}
    __device__ __forceinline__ uint32_t word(long long w) const {
        const uint32_t b = bits[w];
        const uint32_t va = valid ? valid[w] : ~0u;
        uint32_t v = select == MPQE_KG_ROWS_SET ? b : va & ~b;
        if (w == W - 1 && (n & 31)) v &= (1u << (unsigned)(n & 31)) - 1u;
        return v;
    }
};

// csum[i] = the members in the chunks below i, i <= S.chunks: the population counts of the selected words summed per chunk,
// then their exclusive scan over the workgroup; -> csum[S.chunks], the size of the set. csum: KGS_MAX_CHUNKS + 1 ints and
// wsum: KG_SCAN_WAVES ints of the kernel's LDS. Ends on a barrier.
__device__ __forceinline__ int kgs_chunk_sums(const KgsSet &S, int *csum, int *wsum) {
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    for (int c = wave; c < S.chunks; c += KGS_WAVES) {
        const long long w = (long long)c * KGS_CHUNK_WORDS + lane;
        int pc = w < S.W ? __builtin_popcount(S.word(w)) : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) pc += __shfl_xor(pc, o, 64);
        if (lane == 0) csum[c] = pc;
    }
    __syncthreads();
    int own[8], sum = 0;        // thread t owns the 8 entries from 8 t
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        own[i] = 8 * t + i < S.chunks ? csum[8 * t + i] : 0;
        sum += own[i];
    }
    int total;
    int run = kg_workgroup_scan(sum, wsum, total);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (8 * t + i < S.chunks) csum[8 * t + i] = run;
        run += own[i];
    }
    if (t == 0) csum[S.chunks] = total;
    __syncthreads();
    return total;
}

// The row of the member of rank `rank` (< the size of the set): a binary search over the chunk sums, a walk over the chunk's
// words, a select inside the word. -1 (flagged): never.
__device__ __forceinline__ long long kgs_member(const KgsSet &S, const int *csum, int rank, int32_t *err) {
    int a = 0, b = S.chunks;                            // the chunk with csum[a] <= rank < csum[a + 1]
    while (b - a > 1) {
        const int mid = (a + b) >> 1;
        if (csum[mid] <= rank) a = mid; else b = mid;
    }
    rank -= csum[a];
    long long w = (long long)a * KGS_CHUNK_WORDS;
    const long long w_end = w + KGS_CHUNK_WORDS < S.W ? w + KGS_CHUNK_WORDS : S.W;
    uint32_t v = 0u;
    for (; w < w_end; ++w) {
        v = S.word(w);
        const int pc = __builtin_popcount(v);
        if (rank < pc) break;
        rank -= pc;
    }
    if (w >= w_end) {                                   // (never: the sums came from the same words)
        flag_error(err, MPQE_FLAG_INTERNAL);
        return -1;
    }
    for (; rank > 0; --rank) v &= v - 1;
    return w * 32 + __builtin_ctz(v);
}

// min(c, k) members of the set of c into the slots [lo, hi) of rows_out (may be NULL) and, as entity ids through row_ids
// (NULL: -1), of ids_out (may be NULL): all of them ascending, or those of rank P(j), j < k, for the bijection keyed by `key`.
__device__ __forceinline__ void kgs_draw(const KgsSet &S, const int *csum, long long c, unsigned long long key, int k,
                                         long long lo, long long hi, long long *rows_out, long long *ids_out,
                                         const long long *row_ids, int32_t *err) {
    const int t = threadIdx.x;
    const int m = c < k ? (int)c : k;
    if (t == 0 && hi - lo != m) flag_error(err, MPQE_FLAG_BAD_INDEX);
    int h = 1;
    while (((long long)1 << (2 * h)) < c) ++h;
    for (int j = t; j < m; j += KGS_THREADS) {
        if (lo + j >= hi) break;                        // a segment shorter than the list: flagged above
        const long long row = kgs_member(S, csum, (int)(c > k ? kgs_permute(key, c, h, j) : j), err);
        if (row < 0) continue;
        if (rows_out) rows_out[lo + j] = row;
        if (ids_out) ids_out[lo + j] = row_ids ? row_ids[row] : -1;
    }
}

__device__ __forceinline__ unsigned long long kgs_draw_key(unsigned long long seed, long long position) {
    return mpqe_mix64(seed ^ mpqe_mix64((unsigned long long)position));
}

__global__ __launch_bounds__(KGS_THREADS) void kg_sample_rows_kernel(const uint32_t *__restrict__ bits, long long n,
                                                                     const uint32_t *__restrict__ valid, int select,
                                                                     const long long *__restrict__ offsets,
                                                                     long long *__restrict__ rows_out, long long cap, int k,
                                                                     unsigned long long seed, int32_t *err) {
    __shared__ int csum[KGS_MAX_CHUNKS + 1];
    __shared__ int wsum[KG_SCAN_WAVES];
    const long long q = blockIdx.x;
    const long long lo = offsets[q], hi = offsets[q + 1];
    if (lo < 0 || hi < lo || hi > cap) {        // (uniform)
        if (threadIdx.x == 0) flag_error(err, MPQE_FLAG_BAD_INDEX);
        return;
    }
    const KgsSet S(bits + q * ((n + 31) >> 5), valid, select, n);
    const int c = kgs_chunk_sums(S, csum, wsum);
    kgs_draw(S, csum, c, kgs_draw_key(seed, q), k, lo, hi, rows_out, nullptr, nullptr, err);
}

extern "C" int mpqe_kg_sample_rows(const uint32_t *bits, int64_t num_queries, int64_t n, const uint32_t *valid, int select,
                                   const int64_t *offsets, int64_t *rows_out, int64_t rows_cap, int k, uint64_t seed,
                                   int32_t *err, void *stream) {
    if (num_queries < 0 || num_queries > KGS_MAX_SLOTS || n < 1 || rows_cap < 0 || k < 1) return MPQE_ERR_INVALID_ARG;
    if (select != MPQE_KG_ROWS_SET && select != MPQE_KG_ROWS_COMPLEMENT) return MPQE_ERR_INVALID_ARG;
    if (k > KGS_MAX_K || n > KGS_MAX_SAMPLE_ROWS) return MPQE_ERR_UNSUPPORTED;
    if (num_queries == 0) return MPQE_OK;
    if (!bits || !offsets || (rows_cap > 0 && !rows_out)) return MPQE_ERR_INVALID_ARG;
    hipLaunchKernelGGL(kg_sample_rows_kernel, dim3((unsigned)num_queries), dim3(KGS_THREADS), 0, as_stream(stream), bits,
                       (long long)n, valid, select, reinterpret_cast<const long long *>(offsets),
                       reinterpret_cast<long long *>(rows_out), (long long)rows_cap, k, (unsigned long long)seed, err);
    return mpqe_launch_status();
}

// --------------------------------------------------------- at most k members of a set, queries of DIFFERENT modes
// mpqe_kg_sample_rows with n and valid taken per query from mode_of_query [Q] and the index's device table (kg_table.h),
// a row stride for `bits` (the rows of mpqe_kg_answers_mixed: W of the widest mode) and q_base added to the query's
// position in the draw key, so a batch cut into chunks draws what the whole batch draws. ids_out: the same lists as entity
// ids, through the table's row -> id arrays.
__global__ __launch_bounds__(KGS_THREADS) void kg_sample_rows_mixed_kernel(
    const char *__restrict__ table, const uint32_t *__restrict__ bits, long long stride,
    const int32_t *__restrict__ mode_of_query, long long q_base, int select, const long long *__restrict__ offsets,
    long long *__restrict__ rows_out, long long *__restrict__ ids_out, long long cap, int k, unsigned long long seed,
    int32_t *err) {
    __shared__ int csum[KGS_MAX_CHUNKS + 1];
    __shared__ int wsum[KG_SCAN_WAVES];
    const long long q = blockIdx.x;
    const int t = threadIdx.x;
    const KgtHead &H = *kgt_head(table);
    const long long lo = offsets[q], hi = offsets[q + 1];
    const int mode = mode_of_query[q];
    if (lo < 0 || hi < lo || hi > cap || H.magic != KGT_MAGIC || mode < -1 || mode >= H.num_modes) {     // (uniform)
        if (t == 0) flag_error(err, MPQE_FLAG_BAD_INDEX);
        return;
    }
    if (mode < 0) {             // a query that produced nothing: its segment must be empty
        if (t == 0 && hi != lo) flag_error(err, MPQE_FLAG_BAD_INDEX);
        return;
    }
    const long long n = H.mode_rows[mode];
    if (n < 1 || n > KGS_MAX_SAMPLE_ROWS || ((n + 31) >> 5) > stride) {     // (uniform; the host checked its own copy of the modes)
        if (t == 0) flag_error(err, MPQE_FLAG_BAD_INDEX);
        return;
    }
    const KgsSet S(bits + q * stride, H.valid[mode], select, n);
    const int c = kgs_chunk_sums(S, csum, wsum);
    kgs_draw(S, csum, c, kgs_draw_key(seed, q_base + q), k, lo, hi, rows_out, ids_out, H.row_ids[mode], err);
}

extern "C" int mpqe_kg_sample_rows_mixed(const void *table, const int64_t *mode_rows_host, int num_modes,
                                         const uint32_t *bits, int64_t bits_stride, const int32_t *mode_of_query,
                                         int64_t num_queries, int64_t q_base, int select, const int64_t *offsets,
                                         int64_t *rows_out, int64_t *ids_out, int64_t rows_cap, int k, uint64_t seed,
                                         int32_t *err, void *stream) {
    if (num_queries < 0 || num_queries > KGS_MAX_SLOTS || q_base < 0 || rows_cap < 0 || k < 1) return MPQE_ERR_INVALID_ARG;
    if (select != MPQE_KG_ROWS_SET && select != MPQE_KG_ROWS_COMPLEMENT) return MPQE_ERR_INVALID_ARG;
    const int64_t widest = kgt_widest_mode(mode_rows_host, num_modes);
    if (widest == 0) return MPQE_ERR_INVALID_ARG;
    if (k > KGS_MAX_K || widest > KGS_MAX_SAMPLE_ROWS) return MPQE_ERR_UNSUPPORTED;
    if (bits_stride < (widest + 31) / 32) return MPQE_ERR_INVALID_ARG;
    if (num_queries == 0) return MPQE_OK;
    if (!table || ((uintptr_t)table & 7) || !bits || !mode_of_query || !offsets) return MPQE_ERR_INVALID_ARG;
    if (rows_cap > 0 && !rows_out && !ids_out) return MPQE_ERR_INVALID_ARG;
    hipLaunchKernelGGL(kg_sample_rows_mixed_kernel, dim3((unsigned)num_queries), dim3(KGS_THREADS), 0, as_stream(stream),
                       reinterpret_cast<const char *>(table), bits, (long long)bits_stride, mode_of_query, (long long)q_base,
                       select, reinterpret_cast<const long long *>(offsets), reinterpret_cast<long long *>(rows_out),
                       reinterpret_cast<long long *>(ids_out), (long long)rows_cap, k, (unsigned long long)seed, err);
    return mpqe_launch_status();
}
