// Training on R-GCN queries of different formulas at once: mpqe_rgcn_fwd_mixed_save and mpqe_rgcn_bwd_mixed
// (include/mpqe_amd.h). Included by rgcn_mixed.hip after the mixed forward (RgcnMixDesc, RgcnMixArgs, RgcnMixLayers,
// rm_stretch, rm_score_pair and rgcn_mixed_encode_kernel<MODE, 1> are its). The reductions are mix_grad_core.h's.
//
// The workspace (mpqe_rgcn_mixed_train_workspace_bytes; every block a multiple of 256 bytes), Q queries, n pairs, N node
// slots, P passes:
//   S[p], p = 0 .. P  [Q * N, D]  the node states: S[0] the node rows, S[p + 1] what pass p wrote (under the target-message
//                                 readout the last one holds the target slot alone)
//   q_out             [Q, D]
//   G[p], p = 0 .. P  [Q * N, D]  the gradient of S[p]; for 0 < p < P masked by S[p] > 0 on the way out, so G[p + 1] is the
//                                 gradient of pass p's pre-activation. G[P] under the target-message readout: the target
//                                 slot alone -- the other slots are never read (live_out of tmpl_bwd_x_tile, key "none").
//   gq                [Q, D]      the gradient of q_out (the score phase's; under grad_q the caller's buffer is read)
//   GE, GQP           [n, D]      per pair: the gradient of its normalised row, its term of the gq row
//   key, etab         [A * Q + n] the entries' (table index << 40 | row) keys (-1: none) and tables: the anchors in
//                                 (slot, query) order, then the pairs in pair order
//   ptr               [T + 1 + 3 L] the caller's gradient buffers: tables, mode embeddings, basis / root / bias per layer
//   qok               [Q] bytes   1: a stretch of a valid formula ran the query's backward
//   ckey, skey / sval [NC]      the contributions' keys, and keys / contribution numbers sorted; seg [keys][2]; the radix
//                                 sort's scratch
// A stretch writes only the rows of its own queries; a row of a query without qok is never read.
//
// State gradients (rgcn_bwd_mixed_kernel), one launch, a workgroup per stretch: the cosine backward of the stretch's pairs,
// a pair per wave (cosine_bwd_kernel's expressions over pair_cosine's sums), then per query the sum of its pairs' terms in
// the order target, negatives in CSR order; the readout backward (readout_bwd_kernel's; max: the lowest node on ties, from
// S[P]); per pass from the last one tmpl_bwd_x_tile call per node slot and 64-column tile with B = the stretch length and
// b0 = 0; the keys of the entries the stretch owns.
//
// Parameter gradients (param_reduce / vec_reduce with chunks of MPQE_RGCN_MIX_GRAD_CHUNK): contribution c = slot * Q +
// query, the slots per pass the template's edges in edge order then the node slots (the root term), after all passes the
// variable slots (the mode embeddings). Keys: layer * (R + 1) + relation (R: the root), then KP + mode-embedding row, then
// "none" (a query without qok, a slot the target-message skip left out). The sort is stable, so a segment is in (pass,
// slot, query) order. A matrix contribution's A / B rows are its S / G rows; the bias of a layer is the column sum of the
// G rows of its root segment, a mode-embedding row that of the G[0] rows of its variable slots.
//
// Table rows (rgcn_rows_mixed_kernel; rows_reduce): the entries' gradient rows are the anchors' rows of G[0], then GE.
#pragma once
#include "radix_sort.h"

struct RgcnMixIdx {
    int atab[3];        // table index of every anchor slot
    int ttab;           // the target mode's
    int rel[3];         // relation of every template edge
    int var[3];         // mode-embedding row of every variable slot
};

struct RgcnMixTrain {
    const RgcnMixIdx *idx;
    const long long *ids, *neg_off;
    long long n;                        // pairs (0: none are scored)
    const float *gs, *gq_in;            // exactly one
    float eps;
    int L, M, T;                        // layers, mode-embedding rows, tables
    int lop[RM_PASSES];                 // layer of every pass
    unsigned srcs, dsts;                // 2 bits per template edge
    float *S, *Gd;                      // S[p] = S + p * sstride, G[p] = Gd + p * sstride
    long long sstride;
    float *gq, *GE, *GQP;
    long long *key;
    const float **etab;
    float **ptr;
    unsigned char *qok;
    unsigned *ckey, *skey;
    int *sval, *seg;
    long long NC;
    int KP, slots;                      // parameter keys L * (R + 1); contribution slots per pass E + N
};

struct RgcnMixLayout {
    size_t s_off, q_off, g_off, gq_off, ge_off, gqp_off, key_off, etab_off, ptr_off, qok_off, ckey_off, skey_off,
        sval_off, seg_off, sort_off, total;
    long long NC, n_ent;
    int keys;
};

// the query of negative j (neg_off [Q + 1] CSR), or -1 where the offsets do not hold it
__device__ __forceinline__ long long rt_query_of(const long long *__restrict__ neg_off, long long Q, long long j) {
    long long lo = 0, hi = Q;
    while (hi - lo > 1) {
        const long long mid = lo + (hi - lo) / 2;
        if (neg_off[mid] <= j) lo = mid;
        else hi = mid;
    }
    return (neg_off[lo] <= j && j < neg_off[lo + 1]) ? lo : -1;
}

// mpqe_rgcn_fwd_mixed_save's score launch: rgcn_mixed_score_kernel with the query of a pair taken from neg_off
__global__ __launch_bounds__(256) void rgcn_mixed_score_off_kernel(RgcnMixArgs G, const long long *__restrict__ ids,
                                                                   const long long *__restrict__ neg_off, long long n,
                                                                   float eps, float *__restrict__ scores) {
    const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i < n) rm_score_pair(G, ids, i, i < G.Q ? i : rt_query_of(neg_off, G.Q, i - G.Q), eps, scores);
}

// the key of a looked-up row: (table index << 40) | row; -1 where the table wants no gradient or the id is bad
__device__ __forceinline__ long long rt_key(const RgcnMixArgs &G, const RgcnMixTrain &Tn, int tidx, long long id,
                                            long long rows) {
    if (tidx < 0 || tidx >= Tn.T || !Tn.ptr[tidx]) return -1;
    const long long row = lookup_row(G.node_map, G.map_len, id, rows, nullptr);        // (flagged by the forward)
    return row < 0 ? -1 : (((long long)tidx << 40) | row);
}

// one pair's cosine backward by one wave: its term of the gq row -> GQP[i], the gradient of its normalised row -> GE[i]
__device__ __forceinline__ void rt_pair_bwd(const RgcnMixArgs &G, const RgcnMixTrain &Tn, const RgcnMixDesc *M, int tidx,
                                            long long i, long long q, int lane) {
    const int D = G.D;
    const long long row = lookup_row(G.node_map, G.map_len, Tn.ids[i], M->trows, nullptr);
    const float *qi = G.q_out + q * D, *v = M->ttab + (row < 0 ? 0 : row) * D;
    const PairCosine p = pair_cosine(qi, M->ttab, row, D, lane);
    // cosine_bwd_kernel
    const float rq = sqrtf(p.qq), rt = sqrtf(p.tt);
    const float nq = fmaxf(rq, Tn.eps), nt = fmaxf(rt, Tn.eps);
    const float inv = 1.f / (nq * nt);
    const float s = p.dot * inv;
    const float g = Tn.gs[i];
    const float kq = rq > Tn.eps ? s / (nq * nq) : 0.f;
    const float kt = rt > Tn.eps ? s / (nt * nt) : 0.f;
    for (int c = lane; c < D; c += 64) {
        const float a = gload1(qi + c);
        float b = 0.f;
        if (row >= 0) b = gload1(v + c) / p.nrm;
        Tn.GQP[i * D + c] = g * (b * inv - kq * a);
        Tn.GE[i * D + c] = g * (a * inv - kt * b);
    }
    if (lane == 0) {
        const long long at = (long long)G.A * G.Q + i;
        Tn.key[at] = (row < 0 || tidx < 0 || tidx >= Tn.T || !Tn.ptr[tidx]) ? -1 : (((long long)tidx << 40) | row);
        Tn.etab[at] = M->ttab;
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void rgcn_bwd_mixed_kernel(RgcnMixArgs G, RgcnMixLayers W, RgcnMixTrain Tn) {
    __shared__ __attribute__((aligned(16))) float smem[GT_SMEM_FLOATS];
    __shared__ int off_bad;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long first, end;
    int fi;
    if (!rm_stretch(G, first, end, fi)) return;
    fi = __builtin_amdgcn_readfirstlane(fi);
    const int D = G.D, N = G.tp.N, A = G.A, P = G.passes;
    const int Bs = __builtin_amdgcn_readfirstlane((int)(end - first));
    // (no state, no contribution, no entry for a stretch that leaves here: qok and the entries' keys say so)
    if (fi < 0) {
        if (threadIdx.x == 0) flag_error(G.err, MPQE_FLAG_BAD_INDEX);
        return;
    }
    TmplArgs tp = G.tp;
    const RgcnMixDesc *M = G.desc + fi;
    const RgcnMixIdx *I = Tn.idx + fi;
    tp.rel[0] = M->rel[0];
    tp.rel[1] = M->rel[1];
    tp.rel[2] = M->rel[2];
    const bool rel_ok = (tp.E < 1 || (tp.rel[0] >= 0 && tp.rel[0] < G.R)) && (tp.E < 2 || (tp.rel[1] >= 0 && tp.rel[1] < G.R)) &&
                        (tp.E < 3 || (tp.rel[2] >= 0 && tp.rel[2] < G.R));
    if (!rel_ok) {
        if (threadIdx.x == 0) flag_error(G.err, MPQE_FLAG_BAD_RELATION);
        return;
    }
    const float *gq = Tn.gq_in;
    if (Tn.gs) {
        // the stretch's negatives: offsets that do not ascend inside [0, n - Q] are refused for the whole stretch
        const long long nneg = Tn.n - G.Q;
        if (threadIdx.x == 0) off_bad = 0;
        __syncthreads();
        if ((int)threadIdx.x < Bs) {
            const long long a = Tn.neg_off[first + threadIdx.x], b = Tn.neg_off[first + threadIdx.x + 1];
            if (a < 0 || b < a || b > nneg) off_bad = 1;
        }
        __syncthreads();
        if (off_bad) {
            if (threadIdx.x == 0) flag_error(G.err, MPQE_FLAG_BAD_INDEX);
            return;
        }
        const long long a0 = Tn.neg_off[first], b0 = Tn.neg_off[end];
        const long long items = Bs + (b0 - a0);
        for (long long t = wave; t < items; t += 4) {
            long long i, q;
            if (t < Bs) {
                i = q = first + t;
            } else {
                const long long j = a0 + (t - Bs);
                i = G.Q + j;
                // (the offsets ascend inside the stretch: the search stays in it)
                long long lo = first, hi = end;
                while (hi - lo > 1) {
                    const long long mid = lo + (hi - lo) / 2;
                    if (Tn.neg_off[mid] <= j) lo = mid;
                    else hi = mid;
                }
                q = lo;
            }
            rt_pair_bwd(G, Tn, M, I->ttab, i, q, lane);
        }
        __syncthreads();
        // the gq rows: target, then the negatives in CSR order
        for (int e = threadIdx.x; e < Bs * D; e += 256) {
            const int b = e / D, c = e - b * D;
            const long long q = first + b;
            float acc = Tn.GQP[q * D + c];
            const long long hi = Tn.neg_off[q + 1];
            for (long long j = Tn.neg_off[q]; j < hi; ++j) acc += Tn.GQP[(G.Q + j) * D + c];
            Tn.gq[q * D + c] = acc;
        }
        __syncthreads();
        gq = Tn.gq;
    }

    // readout backward -> G[P]
    {
        float *gl = Tn.Gd + (long long)P * Tn.sstride + first * N * D;
        const float *sl = Tn.S + (long long)P * Tn.sstride + first * N * D;
        for (int e = threadIdx.x; e < Bs * D; e += 256) {
            const int b = e / D, c = e - b * D;
            const float gv = gq[(first + b) * D + c];
            float *po = gl + ((long long)b * N) * D + c;
            if (G.readout == MPQE_READOUT_TM) {
                po[(long long)A * D] = gv;
            } else if (G.readout == MPQE_READOUT_SUM) {
                for (int n = 0; n < N; ++n) po[(long long)n * D] = gv;
            } else {
                const float *pr = sl + ((long long)b * N) * D + c;
                float best = pr[0];
                int arg = 0;
                for (int n = 1; n < N; ++n) {
                    const float u = pr[(long long)n * D];
                    if (u > best) {
                        best = u;
                        arg = n;
                    }
                }
                for (int n = 0; n < N; ++n) po[(long long)n * D] = n == arg ? gv : 0.f;
            }
        }
    }
    __syncthreads();

    for (int p = P - 1; p >= 0; --p) {
        const float *basis = W.basis[p], *root = W.root[p];
        const bool tm_last = p == P - 1 && G.readout == MPQE_READOUT_TM;
        const float *gn = Tn.Gd + (long long)(p + 1) * Tn.sstride + first * N * D;
        float *gc = Tn.Gd + (long long)p * Tn.sstride + first * N * D;
        // (S[p], p > 0, is a ReLU output: the gradient is masked on the way out)
        const float *mask = p > 0 ? Tn.S + (long long)p * Tn.sstride + first * N * D : nullptr;
        for (int m = 0; m < N; ++m) {
            // (the target-message readout: the last pass wrote the target slot alone, only its K-blocks are live)
            const bool has = !tm_last || m == A || (tp.E > 0 && tp.src[0] == m && tp.dst[0] == A) ||
                             (tp.E > 1 && tp.src[1] == m && tp.dst[1] == A) || (tp.E > 2 && tp.src[2] == m && tp.dst[2] == A);
            if (!has) {
                for (int e = threadIdx.x; e < Bs * D; e += 256) {
                    const int b = e / D, c = e - b * D;
                    gc[((long long)b * N + m) * D + c] = 0.f;
                }
                continue;
            }
            for (int n0 = 0; n0 < D; n0 += GT_BN)
                tmpl_bwd_x_tile<MODE>(tp, (long long)Bs, gn, nullptr, basis, root, D, D, 0, gc, m, 0ll, n0, smem, mask,
                                      tm_last ? (1u << A) : 0xFu);
        }
        __syncthreads();
    }

    // the anchors' entries; the queries of this stretch have states and gradients
    if ((int)threadIdx.x < Bs * A) {
        const int b = threadIdx.x / A, a = threadIdx.x - b * A;
        const long long q = first + b, at = (long long)a * G.Q + q;
        Tn.key[at] = rt_key(G, Tn, I->atab[a], G.anchors[q * A + a], M->arows[a]);
        Tn.etab[at] = M->atab[a];
    }
    if ((int)threadIdx.x < Bs) Tn.qok[first + threadIdx.x] = 1;
}

// rows_reduce's entries: the anchors in (slot, query) order, then the pairs. (A record of values with ONE base pointer:
// a choice between two pointer members of a record behind references went through scratch.)
struct RgcnMixEntries {
    const long long *key;
    const float *const *etab;
    float *const *ptr;
    const float *G0;
    long long ge_at, Q, na;     // GE's place from G[0], in floats (both lie in the workspace); queries; anchor entries
    int N, D;
    __device__ __forceinline__ const long long *keys() const { return key; }
    __device__ __forceinline__ void tables(long long e, long long k, const float *&tab, float *&gtab) const {
        tab = etab[e];
        gtab = ptr[k >> 40];
    }
    // the anchors' rows of G[0], then GE
    __device__ __forceinline__ const float *grad_row(long long e) const {
        if (e >= na) return G0 + ge_at + (e - na) * D;
        const long long a = e / Q, q = e - a * Q;
        return G0 + (q * N + a) * D;
    }
};

__global__ __launch_bounds__(256) void rgcn_rows_mixed_kernel(RgcnMixArgs G, RgcnMixTrain Tn, long long n_ent) {
    const RgcnMixEntries E = {Tn.key, Tn.etab, Tn.ptr, Tn.Gd, Tn.GE - Tn.Gd, G.Q, (long long)G.A * G.Q, G.tp.N, G.D};
    rows_reduce(E, n_ent, G.D);
}

// contribution c = slot * Q + query -> its key (none: KP + M); the sort numbers the contributions itself
__global__ __launch_bounds__(256) void rgcn_mix_ckeys_kernel(RgcnMixArgs G, RgcnMixTrain Tn) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= Tn.NC) return;
    const int s = (int)(c / G.Q);
    const long long q = c - (long long)s * G.Q;
    const int none = Tn.KP + Tn.M;
    int key = none;
    if (Tn.qok[q]) {
        const RgcnMixIdx &I = Tn.idx[G.fo[q]];
        const int E = G.tp.E, A = G.A;
        if (s < G.passes * Tn.slots) {
            const int p = s / Tn.slots, j = s - p * Tn.slots;
            const bool tm_last = p == G.passes - 1 && G.readout == MPQE_READOUT_TM;
            const int dst = j < E ? (int)((Tn.dsts >> (2 * j)) & 3u) : j - E;
            const int rel = j < E ? (j == 0 ? I.rel[0] : j == 1 ? I.rel[1] : I.rel[2]) : (int)G.R;
            if (!(tm_last && dst != A) && rel >= 0 && rel <= G.R) key = Tn.lop[p] * ((int)G.R + 1) + rel;
        } else {
            const int k = s - G.passes * Tn.slots;
            const int r = k == 0 ? I.var[0] : k == 1 ? I.var[1] : I.var[2];
            if (r >= 0 && r < Tn.M) key = Tn.KP + r;
        }
    }
    Tn.ckey[c] = (unsigned)key;
}

__global__ __launch_bounds__(256) void rgcn_mix_seg_kernel(RgcnMixTrain Tn) {
    mix_seg(Tn.skey, Tn.seg, Tn.NC, (unsigned)(Tn.KP + Tn.M));
}

// sorted value = contribution number
struct RgcnMixContrib {
    const RgcnMixArgs &G;
    const RgcnMixTrain &Tn;
    bool is_bias;       // (term) the vector is a bias, not a mode-embedding row
    // a pass's contribution -> its S row (the A operand) and G row (the B operand)
    __device__ __forceinline__ void rows(unsigned c, const float *&x, const float *&g) const {
        const unsigned Q = (unsigned)G.Q;
        const unsigned s = c / Q, q = c - s * Q;
        const unsigned p = s / (unsigned)Tn.slots, j = s - p * (unsigned)Tn.slots;
        const unsigned E = (unsigned)G.tp.E;
        const unsigned src = j < E ? (Tn.srcs >> (2 * j)) & 3u : j - E, dst = j < E ? (Tn.dsts >> (2 * j)) & 3u : j - E;
        x = Tn.S + (long long)p * Tn.sstride + ((long long)q * G.tp.N + src) * G.D;
        g = Tn.Gd + (long long)(p + 1) * Tn.sstride + ((long long)q * G.tp.N + dst) * G.D;
    }
    // a bias: the G row of a root contribution; a mode-embedding row: the G[0] row of the variable slot
    __device__ __forceinline__ const float *term(unsigned c) const {
        if (is_bias) {
            const float *x, *g;
            rows(c, x, g);
            return g;
        }
        const unsigned Q = (unsigned)G.Q;
        const unsigned s = c / Q, q = c - s * Q;
        return Tn.Gd + ((long long)q * G.tp.N + G.A + (s - (unsigned)(G.passes * Tn.slots))) * G.D;
    }
};

// workgroup = (matrix key, strip of 16 gradient rows)
__global__ __launch_bounds__(256) void rgcn_mix_param_kernel(RgcnMixArgs G, RgcnMixTrain Tn) {
    const int D = G.D, nstrip = D / 16;
    const int par = blockIdx.x / nstrip, rs = blockIdx.x % nstrip;
    const int layer = par / ((int)G.R + 1), rel = par - layer * ((int)G.R + 1);
    float *g = rel < G.R ? Tn.ptr[Tn.T + 1 + layer] : Tn.ptr[Tn.T + 1 + Tn.L + layer];
    if (!g) return;
    if (rel < G.R) g += (long long)rel * D * D;
    const int lo = Tn.seg[2 * par], hi = Tn.seg[2 * par + 1];
    if (lo >= hi) return;
    param_reduce<MPQE_RGCN_MIX_GRAD_CHUNK>(lo, hi, rs, g, D, Tn.sval, RgcnMixContrib{G, Tn, false});
}

// workgroup = one vector: the bias of layer k (k < L) or mode-embedding row k - L
__global__ __launch_bounds__(256) void rgcn_mix_vec_kernel(RgcnMixArgs G, RgcnMixTrain Tn) {
    const int D = G.D, k = blockIdx.x;
    const bool is_bias = k < Tn.L;
    float *g = is_bias ? Tn.ptr[Tn.T + 1 + 2 * Tn.L + k] : Tn.ptr[Tn.T];
    if (!g) return;
    if (!is_bias) g += (long long)(k - Tn.L) * D;
    const int key = is_bias ? k * ((int)G.R + 1) + (int)G.R : Tn.KP + (k - Tn.L);
    const int lo = Tn.seg[2 * key], hi = Tn.seg[2 * key + 1];
    if (lo >= hi) return;
    vec_reduce<MPQE_RGCN_MIX_GRAD_CHUNK>(lo, hi, g, D, Tn.sval, RgcnMixContrib{G, Tn, is_bias});
}

// ------------------------------------------------------------------------------------------------ host side
static inline size_t rt_index_size(int64_t F) { return align_up((size_t)F * sizeof(RgcnMixIdx), 256); }

extern "C" size_t mpqe_rgcn_mixed_index_bytes(int64_t num_formulas) {
    return rm_formulas_ok(num_formulas) ? rt_index_size(num_formulas) : 0;
}

extern "C" int mpqe_rgcn_mixed_index_build(int query_type, const int32_t *recs_host, int64_t num_formulas, void *index,
                                           size_t index_bytes, void *stream) {
    if (query_type < 0 || query_type >= MPQE_Q_COUNT || !recs_host || !index) return MPQE_ERR_INVALID_ARG;
    if (!rm_formulas_ok(num_formulas) || (uintptr_t)index % 256 != 0) return MPQE_ERR_INVALID_ARG;
    const TemplateDesc &d = kTemplates[query_type];
    return mix_upload<RgcnMixIdx>(index, (size_t)num_formulas, as_stream(stream), [&](RgcnMixIdx *image) -> int {
        memset(image, 0, (size_t)num_formulas * sizeof(RgcnMixIdx));
        for (int64_t f = 0; f < num_formulas; ++f) {
            const int32_t *rec = recs_host + f * MPQE_RGCN_MIX_REC_INTS;
            RgcnMixIdx &I = image[f];
            bool bad = false;
            auto take = [&](int32_t v) {
                bad = bad || v < 0;
                return v;
            };
            for (int e = 0; e < d.E; ++e) I.rel[e] = take(rec[e]);
            for (int a = 0; a < d.A; ++a) I.atab[a] = take(rec[3 + a]);
            for (int k = 0; k < d.V; ++k) I.var[k] = take(rec[6 + k]);
            I.ttab = take(rec[9]);
            if (bad) return MPQE_ERR_INVALID_ARG;
        }
        return index_bytes < rt_index_size(num_formulas) ? MPQE_ERR_WORKSPACE : MPQE_OK;
    });
}

// the shapes the training entries cover
static inline bool rt_shape_ok(int64_t D, int passes, int readout) {
    return D >= 16 && D <= 256 && D % 16 == 0 && passes >= 1 && passes <= RM_PASSES &&
           (readout == MPQE_READOUT_SUM || readout == MPQE_READOUT_MAX || readout == MPQE_READOUT_TM);
}

// 0: fine; the sizes out of range otherwise
static int rt_layout(int query_type, int64_t Q, int64_t n, int64_t D, int passes, int64_t R, int T, int64_t M, int L,
                     RgcnMixLayout *Y) {
    if (query_type < 0 || query_type >= MPQE_Q_COUNT || Q < 1 || Q >= ((int64_t)1 << 25)) return MPQE_ERR_INVALID_ARG;
    if (n < 0 || (n > 0 && n < Q) || R < 1 || T < 1 || M < 1 || L < 1) return MPQE_ERR_INVALID_ARG;
    if (D < 16 || D > 256 || D % 16 != 0 || passes < 1 || passes > RM_PASSES) return MPQE_ERR_UNSUPPORTED;
    if (n >= ((int64_t)1 << 31) || L > RM_PASSES || T > (1 << 20) || M > (1 << 24) || R > (1 << 24)) return MPQE_ERR_UNSUPPORTED;
    const TemplateDesc &d = kTemplates[query_type];
    const long long keys = (long long)L * (R + 1) + M + 1;
    const long long NC = ((long long)passes * (d.E + d.N) + d.V) * Q;
    if (keys >= (1ll << 28) || NC >= (1ll << 30)) return MPQE_ERR_UNSUPPORTED;
    memset(Y, 0, sizeof(*Y));
    Y->NC = NC;
    Y->keys = (int)keys;
    Y->n_ent = (long long)d.A * Q + n;
    const size_t sb = rm_state_bytes(d, Q, D), ob = rm_out_bytes(Q, D), pb = align_up((size_t)n * (size_t)D * 4, 256);
    size_t off = 0;
    Y->s_off = off;
    off += (size_t)(passes + 1) * sb;
    Y->q_off = off;
    off += ob;
    Y->g_off = off;
    off += (size_t)(passes + 1) * sb;
    Y->gq_off = off;
    off += ob;
    Y->ge_off = off;
    off += pb;
    Y->gqp_off = off;
    off += pb;
    Y->key_off = off;
    off += align_up((size_t)Y->n_ent * 8, 256);
    Y->etab_off = off;
    off += align_up((size_t)Y->n_ent * 8, 256);
    Y->ptr_off = off;
    off += align_up((size_t)(T + 1 + 3 * L) * 8, 256);
    Y->qok_off = off;
    off += align_up((size_t)Q, 256);
    const size_t cb = align_up((size_t)NC * 4, 256);
    Y->ckey_off = off;
    Y->skey_off = off + cb;
    Y->sval_off = off + 2 * cb;
    off += 3 * cb;
    Y->seg_off = off;
    off += align_up((size_t)keys * 8, 256);
    Y->sort_off = off;
    Y->total = off + radix_sort_tmp_bytes<unsigned>(NC);
    return MPQE_OK;
}

extern "C" size_t mpqe_rgcn_mixed_train_workspace_bytes(int query_type, int64_t num_queries, int64_t n, int64_t dim, int passes,
                                                        int64_t num_relations, int num_tables, int64_t mode_emb_rows,
                                                        int num_layers) {
    RgcnMixLayout Y;
    if (rt_layout(query_type, num_queries, n, dim, passes, num_relations, num_tables, mode_emb_rows, num_layers, &Y) != MPQE_OK)
        return 0;
    return Y.total;
}

// Everything the save call and the backward check alike, the kernels' records. *empty: no queries, nothing to launch.
static int rt_call(int query_type, int64_t num_formulas, const void *desc, size_t desc_bytes, const int64_t *node_map,
                   int64_t node_map_len, const float *mode_emb, const float *const *basis_host, const float *const *root_host,
                   const float *const *bias_host, int64_t num_relations, int passes, int readout, int64_t dim,
                   const int64_t *formula_of, const int64_t *anchors, int64_t num_queries, int64_t n, int num_tables,
                   int64_t mode_emb_rows, int num_layers, void *workspace, size_t workspace_bytes, int32_t *err,
                   RgcnMixArgs *Gp, RgcnMixLayers *Wp, RgcnMixLayout *Y, bool *empty) {
    *empty = false;
    if (query_type < 0 || query_type >= MPQE_Q_COUNT || num_queries < 0 || node_map_len < 0 || dim <= 0 || num_relations < 1)
        return MPQE_ERR_INVALID_ARG;
    if (!rm_formulas_ok(num_formulas)) return MPQE_ERR_INVALID_ARG;
    if (!desc || (uintptr_t)desc % 256 != 0 || !basis_host || !root_host) return MPQE_ERR_INVALID_ARG;
    if (n < 0 || num_tables < 1 || mode_emb_rows < 1 || num_layers < 1) return MPQE_ERR_INVALID_ARG;
    if (!rt_shape_ok(dim, passes, readout) || num_layers > RM_PASSES) return MPQE_ERR_UNSUPPORTED;
    RgcnMixLayers &W = *Wp;
    memset(&W, 0, sizeof(W));
    for (int p = 0; p < passes; ++p) {
        if (!basis_host[p] || !root_host[p]) return MPQE_ERR_INVALID_ARG;
        if ((uintptr_t)basis_host[p] % 16 != 0 || (uintptr_t)root_host[p] % 16 != 0) return MPQE_ERR_UNSUPPORTED;
        W.basis[p] = basis_host[p];
        W.root[p] = root_host[p];
        W.bias[p] = bias_host ? bias_host[p] : nullptr;
    }
    if (desc_bytes < rm_desc_size(num_formulas)) return MPQE_ERR_WORKSPACE;
    if (num_queries == 0) {
        *empty = true;
        return n == 0 ? MPQE_OK : MPQE_ERR_INVALID_ARG;
    }
    if (!mode_emb || !formula_of || !anchors || !workspace) return MPQE_ERR_INVALID_ARG;
    if ((uintptr_t)mode_emb % 16 != 0) return MPQE_ERR_UNSUPPORTED;
    if ((uintptr_t)workspace % 256 != 0) return MPQE_ERR_INVALID_ARG;
    const int st = rt_layout(query_type, num_queries, n, dim, passes, num_relations, num_tables, mode_emb_rows, num_layers, Y);
    if (st != MPQE_OK) return st;
    if (workspace_bytes < Y->total) return MPQE_ERR_WORKSPACE;
    const TemplateDesc &d = kTemplates[query_type];
    RgcnMixArgs &G = *Gp;
    memset(&G, 0, sizeof(G));
    G.tp.N = d.N;
    G.tp.E = d.E;
    for (int e = 0; e < 3; ++e) {
        G.tp.src[e] = e < d.E ? d.src[e] : 0;
        G.tp.dst[e] = e < d.E ? d.dst[e] : 0;
    }
    G.A = d.A;
    G.V = d.V;
    G.D = (int)dim;
    G.passes = passes;
    G.readout = readout;
    G.F = (int)num_formulas;
    G.Q = num_queries;
    G.R = num_relations;
    G.map_len = node_map_len;
    G.desc = reinterpret_cast<const RgcnMixDesc *>(desc);
    G.node_map = reinterpret_cast<const long long *>(node_map);
    G.fo = reinterpret_cast<const long long *>(formula_of);
    G.anchors = reinterpret_cast<const long long *>(anchors);
    G.mode_emb = mode_emb;
    char *wb = reinterpret_cast<char *>(workspace);
    // (the saving encode kernel walks S[p] = s0 + p * (s1 - s0))
    G.s0 = reinterpret_cast<float *>(wb + Y->s_off);
    G.s1 = reinterpret_cast<float *>(wb + Y->s_off + rm_state_bytes(d, num_queries, dim));
    G.q_out = reinterpret_cast<float *>(wb + Y->q_off);
    G.err = err;
    return MPQE_OK;
}

extern "C" int mpqe_rgcn_fwd_mixed_save(int query_type, int64_t num_formulas, const void *desc, size_t desc_bytes,
                                        const int64_t *node_map, int64_t node_map_len, const float *mode_emb,
                                        const float *const *basis_host, const float *const *root_host,
                                        const float *const *bias_host, int64_t num_relations, int passes, int readout,
                                        int64_t dim, const int64_t *formula_of, const int64_t *anchors, int64_t num_queries,
                                        const int64_t *ids, const int64_t *neg_off, int64_t n, float eps, int num_tables,
                                        int64_t mode_emb_rows, int num_layers, void *workspace, size_t workspace_bytes,
                                        float *scores, float *q_out, int32_t *err, void *stream) {
    RgcnMixArgs G;
    RgcnMixLayers W;
    RgcnMixLayout Y;
    bool empty;
    const int st = rt_call(query_type, num_formulas, desc, desc_bytes, node_map, node_map_len, mode_emb, basis_host, root_host,
                           bias_host, num_relations, passes, readout, dim, formula_of, anchors, num_queries, n, num_tables,
                           mode_emb_rows, num_layers, workspace, workspace_bytes, err, &G, &W, &Y, &empty);
    if (st != MPQE_OK || empty) return st;
    if (n > 0 && (!ids || !neg_off || !scores)) return MPQE_ERR_INVALID_ARG;
    if ((uintptr_t)q_out % 16 != 0) return MPQE_ERR_INVALID_ARG;
    hipStream_t s = as_stream(stream);
    const dim3 grid((unsigned)((num_queries + GT_BM - 1) / GT_BM * RM_STRETCHES));
    if (dim % GT_BN == 0)
        hipLaunchKernelGGL((rgcn_mixed_encode_kernel<LD_FAST, 1>), grid, dim3(256), 0, s, G, W);
    else
        hipLaunchKernelGGL((rgcn_mixed_encode_kernel<LD_PRED, 1>), grid, dim3(256), 0, s, G, W);
    if (n > 0)
        hipLaunchKernelGGL(rgcn_mixed_score_off_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, G,
                           reinterpret_cast<const long long *>(ids), reinterpret_cast<const long long *>(neg_off),
                           (long long)n, eps, scores);
    if (q_out && hipMemcpyAsync(q_out, G.q_out, (size_t)num_queries * (size_t)dim * 4, hipMemcpyDeviceToDevice, s) != hipSuccess)
        return MPQE_ERR_LAUNCH;
    return mpqe_launch_status();
}

extern "C" int mpqe_rgcn_bwd_mixed(int query_type, int64_t num_formulas, const void *desc, size_t desc_bytes, const void *index,
                                   size_t index_bytes, const int64_t *node_map, int64_t node_map_len, const float *mode_emb,
                                   const float *const *basis_host, const float *const *root_host,
                                   const float *const *bias_host, int64_t num_relations, int passes, int readout, int64_t dim,
                                   const int64_t *formula_of, const int64_t *anchors, int64_t num_queries, const int64_t *ids,
                                   const int64_t *neg_off, int64_t n, float eps, int num_tables, int64_t mode_emb_rows,
                                   int num_layers, const int *layer_of_pass_host, const float *grad_scores,
                                   const float *grad_q, float *const *grad_tables_host, float *grad_mode_emb,
                                   float *const *grad_basis_host, float *const *grad_root_host,
                                   float *const *grad_bias_host, void *workspace, size_t workspace_bytes, int32_t *err,
                                   void *stream) {
    if (!index || (uintptr_t)index % 256 != 0 || !layer_of_pass_host) return MPQE_ERR_INVALID_ARG;
    if ((grad_scores != nullptr) == (grad_q != nullptr)) return MPQE_ERR_INVALID_ARG;
    if (rm_formulas_ok(num_formulas) && index_bytes < rt_index_size(num_formulas)) return MPQE_ERR_WORKSPACE;
    RgcnMixArgs G;
    RgcnMixLayers W;
    RgcnMixLayout Y;
    bool empty;
    int st = rt_call(query_type, num_formulas, desc, desc_bytes, node_map, node_map_len, mode_emb, basis_host, root_host,
                     bias_host, num_relations, passes, readout, dim, formula_of, anchors, num_queries, n, num_tables,
                     mode_emb_rows, num_layers, workspace, workspace_bytes, err, &G, &W, &Y, &empty);
    if (st != MPQE_OK || empty) return st;
    if (grad_scores && (n < num_queries || !ids || !neg_off)) return MPQE_ERR_INVALID_ARG;
    if ((uintptr_t)grad_scores % 4 != 0 || (uintptr_t)grad_q % 16 != 0 || (uintptr_t)grad_mode_emb % 16 != 0)
        return MPQE_ERR_INVALID_ARG;
    const TemplateDesc &d = kTemplates[query_type];
    const int T = num_tables, L = num_layers;
    RgcnMixTrain Tn;
    memset(&Tn, 0, sizeof(Tn));
    for (int p = 0; p < passes; ++p) {
        if (layer_of_pass_host[p] < 0 || layer_of_pass_host[p] >= L) return MPQE_ERR_INVALID_ARG;
        Tn.lop[p] = layer_of_pass_host[p];
    }
    bool any_table = false, any_mat = false, any_vec = grad_mode_emb != nullptr;
    hipStream_t s = as_stream(stream);
    char *wb = reinterpret_cast<char *>(workspace);
    st = mix_upload_grad_ptrs(wb + Y.ptr_off, (size_t)T + 1 + 3 * (size_t)L, s, [&](float **image) {
        for (int t = 0; t < T; ++t) {
            image[t] = grad_tables_host ? grad_tables_host[t] : nullptr;
            any_table = any_table || image[t];
        }
        image[T] = grad_mode_emb;
        for (int l = 0; l < L; ++l) {
            image[T + 1 + l] = grad_basis_host ? grad_basis_host[l] : nullptr;
            image[T + 1 + L + l] = grad_root_host ? grad_root_host[l] : nullptr;
            image[T + 1 + 2 * L + l] = grad_bias_host ? grad_bias_host[l] : nullptr;
            any_mat = any_mat || image[T + 1 + l] || image[T + 1 + L + l];
            any_vec = any_vec || image[T + 1 + 2 * L + l];
        }
    });
    if (st != MPQE_OK) return st;
    Tn.idx = reinterpret_cast<const RgcnMixIdx *>(index);
    Tn.ids = reinterpret_cast<const long long *>(ids);
    Tn.neg_off = reinterpret_cast<const long long *>(neg_off);
    Tn.n = grad_scores ? n : 0;
    Tn.gs = grad_scores;
    Tn.gq_in = grad_q;
    Tn.eps = eps;
    Tn.L = L;
    Tn.M = (int)mode_emb_rows;
    Tn.T = T;
    for (int e = 0; e < d.E; ++e) {
        Tn.srcs |= (unsigned)d.src[e] << (2 * e);
        Tn.dsts |= (unsigned)d.dst[e] << (2 * e);
    }
    Tn.S = reinterpret_cast<float *>(wb + Y.s_off);
    Tn.Gd = reinterpret_cast<float *>(wb + Y.g_off);
    Tn.sstride = (long long)(rm_state_bytes(d, num_queries, dim) / 4);
    Tn.gq = reinterpret_cast<float *>(wb + Y.gq_off);
    Tn.GE = reinterpret_cast<float *>(wb + Y.ge_off);
    Tn.GQP = reinterpret_cast<float *>(wb + Y.gqp_off);
    Tn.key = reinterpret_cast<long long *>(wb + Y.key_off);
    Tn.etab = reinterpret_cast<const float **>(wb + Y.etab_off);
    Tn.ptr = reinterpret_cast<float **>(wb + Y.ptr_off);
    Tn.qok = reinterpret_cast<unsigned char *>(wb + Y.qok_off);
    Tn.ckey = reinterpret_cast<unsigned *>(wb + Y.ckey_off);
    Tn.skey = reinterpret_cast<unsigned *>(wb + Y.skey_off);
    Tn.sval = reinterpret_cast<int *>(wb + Y.sval_off);
    Tn.seg = reinterpret_cast<int *>(wb + Y.seg_off);
    Tn.NC = Y.NC;
    Tn.KP = L * ((int)num_relations + 1);
    Tn.slots = d.E + d.N;
    // (every entry and every query a stretch of a valid formula does not own: key -1, qok 0)
    if (hipMemsetAsync(wb + Y.key_off, 0xFF, (size_t)Y.n_ent * 8, s) != hipSuccess) return MPQE_ERR_LAUNCH;
    if (hipMemsetAsync(wb + Y.qok_off, 0, (size_t)num_queries, s) != hipSuccess) return MPQE_ERR_LAUNCH;
    const dim3 grid((unsigned)((num_queries + GT_BM - 1) / GT_BM * RM_STRETCHES));
    if (dim % GT_BN == 0)
        hipLaunchKernelGGL(rgcn_bwd_mixed_kernel<LD_FAST>, grid, dim3(256), 0, s, G, W, Tn);
    else
        hipLaunchKernelGGL(rgcn_bwd_mixed_kernel<LD_PRED>, grid, dim3(256), 0, s, G, W, Tn);
    st = mpqe_launch_status();
    if (st != MPQE_OK) return st;
    if (any_mat || any_vec) {
        if (hipMemsetAsync(wb + Y.seg_off, 0, (size_t)Y.keys * 8, s) != hipSuccess) return MPQE_ERR_LAUNCH;
        const dim3 cgrid((unsigned)((Tn.NC + 255) / 256));
        hipLaunchKernelGGL(rgcn_mix_ckeys_kernel, cgrid, dim3(256), 0, s, G, Tn);
        int bits = 1;
        while ((1ll << bits) < Y.keys) ++bits;
        st = radix_sort_pairs_own<unsigned>(wb + Y.sort_off, Tn.ckey, Tn.skey, nullptr, Tn.sval, Tn.NC, bits, s);
        if (st != MPQE_OK) return st;
        hipLaunchKernelGGL(rgcn_mix_seg_kernel, cgrid, dim3(256), 0, s, Tn);
        if (any_mat)
            hipLaunchKernelGGL(rgcn_mix_param_kernel, dim3((unsigned)((long long)Tn.KP * (dim / 16))), dim3(256), 0, s, G, Tn);
        if (any_vec)
            hipLaunchKernelGGL(rgcn_mix_vec_kernel, dim3((unsigned)(L + (int)mode_emb_rows)), dim3(256), 0, s, G, Tn);
        st = mpqe_launch_status();
        if (st != MPQE_OK) return st;
    }
    if (any_table) {
        const long long n_ent = (long long)d.A * num_queries + Tn.n;
        hipLaunchKernelGGL(rgcn_rows_mixed_kernel, dim3((unsigned)((n_ent + 3) / 4)), dim3(256), 0, s, G, Tn, n_ent);
        st = mpqe_launch_status();
    }
    return st;
}
