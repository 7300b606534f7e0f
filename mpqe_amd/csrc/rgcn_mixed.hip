// R-GCN scores of queries of DIFFERENT formulas of one query type in two launches (include/mpqe_amd.h:
// mpqe_rgcn_embed_mixed / mpqe_rgcn_fwd_mixed; the forward with states and the backward: rgcn_mixed_train.h). The formulas of a query type share the template (N, E, src / dst, the
// variable slots), the pass count, the layers and the readout; a formula's own part -- the relation of every template
// edge, the entity table of every anchor slot, the mode-embedding row of every variable slot, the target mode's table --
// is one RgcnMixDesc in device memory (mpqe_rgcn_mixed_desc_build; addresses and indices only, kept by the caller).
//
// rgcn_mixed_encode_kernel: the queries are cut into blocks of GT_BM (64) and a block into its maximal stretches of one
// formula; workgroup 64 k + j owns the j-th stretch of block k and leaves at once when the block has fewer. Every
// workgroup reads the block's (at most 64) formula indices with uniform loads: no pre-pass, no host read. The workgroup
// runs its stretch's whole programme out of two node-state buffers in the workspace (rows first*N .. end*N of each are
// its own): node rows, then per pass one tmpl_fwd_tile call per node slot and 64-column tile with B = the stretch length
// and b0 = 0, a __syncthreads() between a pass's writes and the next pass's reads, then the readout. An output element is
// the same sequence of MFMA operands as in mpqe_rgcn_template_fwd (the rows that share a tile do not enter it), the node
// rows and the readout are the per-op kernels' expressions, so q_out is the module path's to the bit.
//
// rgcn_mixed_score_kernel: one wave per pair row; the id's table row is normalised in registers (row_norm_store's
// arithmetic, nothing stored) and scored against q_out[qrow] with cosine_fwd_kernel's expressions.
#include <string.h>

#include <new>

#include "mix_grad_core.h"
#include "rgcn_template_body.h"

#define RM_PASSES 4
#define RM_STRETCHES GT_BM      // workgroups per block of GT_BM queries: a block has at most that many stretches

struct RgcnMixDesc {
    const float *atab[3];       // entity table of every anchor slot
    long long arows[3];
    const float *ttab;          // the target mode's table
    long long trows;
    long long rel[3];           // relation of every template edge
    long long var[3];           // mode-embedding row of every variable slot
};

struct RgcnMixLayers {
    const float *basis[RM_PASSES], *root[RM_PASSES], *bias[RM_PASSES];
};

struct RgcnMixArgs {
    TmplArgs tp;                // N, E, src, dst of the query type (rel comes from the descriptor)
    int A, V, D, passes, readout, F;
    long long Q, R, map_len;
    const RgcnMixDesc *desc;
    const long long *node_map, *fo, *anchors;
    const float *mode_emb;
    float *s0, *s1, *q_out;
    int32_t *err;
};

// this workgroup's stretch of queries (mix_find_stretch): workgroup RM_STRETCHES k + j owns the j-th stretch of block k
__device__ __forceinline__ bool rm_stretch(const RgcnMixArgs &G, long long &first, long long &end, int &fi) {
    return mix_find_stretch((long long)(blockIdx.x / RM_STRETCHES) * GT_BM, GT_BM, G.Q, blockIdx.x % RM_STRETCHES,
                            [&](long long q) {
                                const long long k = G.fo[q];
                                return k < 0 || k >= G.F ? -1 : k;
                            },
                            first, end, fi);
}

// SAVE (mpqe_rgcn_fwd_mixed_save, rgcn_mixed_train.h): every pass keeps its state -- pass p reads S[p] and writes S[p + 1],
// S[p] = s0 + p * (s1 - s0) -- in place of the two buffers taking turns.
template <int MODE, int SAVE = 0>
__global__ __launch_bounds__(256) void rgcn_mixed_encode_kernel(RgcnMixArgs G, RgcnMixLayers W) {
    __shared__ __attribute__((aligned(16))) float smem[GT_SMEM_FLOATS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long first, end;
    int fi;
    if (!rm_stretch(G, first, end, fi)) return;
    fi = __builtin_amdgcn_readfirstlane(fi);
    const int D = G.D, N = G.tp.N, A = G.A;
    const int Bs = __builtin_amdgcn_readfirstlane((int)(end - first));
    float *qo = G.q_out + first * D;
    bool bad = fi < 0;
    if (bad && threadIdx.x == 0) flag_error(G.err, MPQE_FLAG_BAD_INDEX);
    TmplArgs tp = G.tp;
    const RgcnMixDesc *M = G.desc + (bad ? 0 : fi);
    if (!bad) {
        tp.rel[0] = M->rel[0];
        tp.rel[1] = M->rel[1];
        tp.rel[2] = M->rel[2];
        // (the relation count belongs to the call, not to the descriptor block: checked here, before any matrix is read)
        const bool rel_ok = (tp.E < 1 || (tp.rel[0] >= 0 && tp.rel[0] < G.R)) && (tp.E < 2 || (tp.rel[1] >= 0 && tp.rel[1] < G.R)) &&
                            (tp.E < 3 || (tp.rel[2] >= 0 && tp.rel[2] < G.R));
        if (!rel_ok) {
            if (threadIdx.x == 0) flag_error(G.err, MPQE_FLAG_BAD_RELATION);
            bad = true;
        }
    }
    if (bad) {      // the stretch's embeddings are zeros: its pairs score 0
        for (int e = threadIdx.x; e < Bs * D; e += 256) qo[e] = 0.f;
        return;
    }
    float *cur = G.s0 + first * N * D, *nxt = G.s1 + first * N * D;

    // node rows: anchors as embed_l2norm_fwd_kernel (one wave per row, 16-byte form), variables as var_rows_fwd_kernel
    for (int r = wave; r < Bs * A; r += 4) {
        const int b = r / A, a = r - b * A;
        const long long rows = M->arows[a];
        const long long row = lookup_row(G.node_map, G.map_len, G.anchors[(first + b) * A + a], rows, lane == 0 ? G.err : nullptr);
        float *o = cur + ((long long)b * N + a) * D;
        if (row < 0) {
            for (int c = lane; c < D; c += 64) o[c] = 0.f;
            continue;
        }
        row_norm_store(M->atab[a] + row * D, o, D, lane, true);
    }
    for (int e = threadIdx.x; e < Bs * G.V * D; e += 256) {
        const int c = e % D;
        const int bk = e / D;
        const int k = bk % G.V, b = bk / G.V;
        cur[((long long)b * N + A + k) * D + c] = G.mode_emb[M->var[k] * D + c];
    }
    __syncthreads();

    for (int p = 0; p < G.passes; ++p) {
        // (W is never written: the index goes straight into the scalar loads from the argument segment)
        const float *basis = W.basis[p], *root = W.root[p], *bias = W.bias[p];
        const bool last = p == G.passes - 1;
        for (int n = 0; n < N; ++n) {
            // (the target-message readout reads the target slot alone: the last pass's other slots have no reader)
            if (last && G.readout == MPQE_READOUT_TM && n != A) continue;
            for (int n0 = 0; n0 < D; n0 += GT_BN)
                tmpl_fwd_tile<MODE>(tp, (long long)Bs, cur, basis, root, bias, D, D, last ? 0 : 1, nxt, n, 0ll, n0, smem);
        }
        __syncthreads();
        if (SAVE) {
            const long long stride = G.s1 - G.s0;
            cur = nxt;
            nxt = nxt + stride;
        } else {
            float *t = cur; cur = nxt; nxt = t;
        }
    }

    // readout: readout_fwd_kernel's expressions (the sum in node order)
    for (int e = threadIdx.x; e < Bs * D; e += 256) {
        const int b = e / D, c = e - b * D;
        const float *pr = cur + ((long long)b * N) * D + c;
        float v;
        if (G.readout == MPQE_READOUT_TM) {
            v = pr[(long long)A * D];
        } else if (G.readout == MPQE_READOUT_SUM) {
            float s = 0.f;
            for (int n = 0; n < N; ++n) s += pr[(long long)n * D];
            v = s;
        } else {
            float best = pr[0];
            for (int n = 1; n < N; ++n) {
                const float u = pr[(long long)n * D];
                if (u > best) best = u;
            }
            v = best;
        }
        qo[e] = v;
    }
}

// pair i of query q by one wave: the cosine of q_out[q] and the id's normalised table row (pair_cosine; the final
// expression is cosine_fwd_kernel's); a query or a formula out of range flags MPQE_FLAG_BAD_INDEX and scores 0
__device__ __forceinline__ void rm_score_pair(const RgcnMixArgs &G, const long long *__restrict__ ids, long long i, long long q,
                                              float eps, float *__restrict__ scores) {
    const int lane = threadIdx.x & 63;
    long long f = -1;
    if (q >= 0 && q < G.Q) f = G.fo[q];
    if (f < 0 || f >= G.F) {
        if (lane == 0) {
            flag_error(G.err, MPQE_FLAG_BAD_INDEX);
            scores[i] = 0.f;
        }
        return;
    }
    const RgcnMixDesc *M = G.desc + f;
    const long long row = lookup_row(G.node_map, G.map_len, ids[i], M->trows, lane == 0 ? G.err : nullptr);
    const PairCosine p = pair_cosine(G.q_out + q * G.D, M->ttab, row, G.D, lane);
    const float nq = fmaxf(sqrtf(p.qq), eps), nt = fmaxf(sqrtf(p.tt), eps);
    if (lane == 0) scores[i] = p.dot / (nq * nt);
}

__global__ __launch_bounds__(256) void rgcn_mixed_score_kernel(RgcnMixArgs G, const long long *__restrict__ ids,
                                                               const long long *__restrict__ qrow, long long n, float eps,
                                                               float *__restrict__ scores) {
    const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i < n) rm_score_pair(G, ids, i, qrow[i], eps, scores);
}

// ------------------------------------------------------------------------------------ host side
static inline bool rm_formulas_ok(int64_t F) { return F >= 1 && F < ((int64_t)1 << 24); }
static inline size_t rm_desc_size(int64_t F) { return align_up((size_t)F * sizeof(RgcnMixDesc), 256); }

extern "C" size_t mpqe_rgcn_mixed_desc_bytes(int64_t num_formulas) {
    return rm_formulas_ok(num_formulas) ? rm_desc_size(num_formulas) : 0;
}

extern "C" int mpqe_rgcn_mixed_desc_build(int query_type, const int32_t *recs_host, int64_t num_formulas,
                                          const float *const *tables_host, const int64_t *table_rows_host, int num_tables,
                                          int64_t mode_emb_rows, void *desc, size_t desc_bytes, void *stream) {
    if (query_type < 0 || query_type >= MPQE_Q_COUNT || !recs_host || !tables_host || !table_rows_host || !desc)
        return MPQE_ERR_INVALID_ARG;
    if (!rm_formulas_ok(num_formulas) || num_tables < 1 || mode_emb_rows < 1) return MPQE_ERR_INVALID_ARG;
    if ((uintptr_t)desc % 256 != 0) return MPQE_ERR_INVALID_ARG;
    const TemplateDesc &d = kTemplates[query_type];
    for (int t = 0; t < num_tables; ++t) {
        if (!tables_host[t] || table_rows_host[t] < 0) return MPQE_ERR_INVALID_ARG;
        if ((uintptr_t)tables_host[t] % 16 != 0) return MPQE_ERR_UNSUPPORTED;
    }
    RgcnMixDesc *image = new (std::nothrow) RgcnMixDesc[(size_t)num_formulas];
    if (!image) return MPQE_ERR_INVALID_ARG;
    memset(image, 0, (size_t)num_formulas * sizeof(RgcnMixDesc));
    int st = MPQE_OK;
    for (int64_t f = 0; f < num_formulas && st == MPQE_OK; ++f) {
        const int32_t *rec = recs_host + f * MPQE_RGCN_MIX_REC_INTS;
        RgcnMixDesc &M = image[f];
        for (int e = 0; e < d.E; ++e) {
            if (rec[e] < 0) st = MPQE_ERR_INVALID_ARG;
            M.rel[e] = rec[e];
        }
        for (int a = 0; a < d.A && st == MPQE_OK; ++a) {
            const int t = rec[3 + a];
            if (t < 0 || t >= num_tables) {
                st = MPQE_ERR_INVALID_ARG;
                break;
            }
            M.atab[a] = tables_host[t];
            M.arows[a] = table_rows_host[t];
        }
        for (int k = 0; k < d.V; ++k) {
            if (rec[6 + k] < 0 || rec[6 + k] >= mode_emb_rows) st = MPQE_ERR_INVALID_ARG;
            M.var[k] = rec[6 + k];
        }
        const int tt = rec[9];
        if (tt < 0 || tt >= num_tables) {
            st = MPQE_ERR_INVALID_ARG;
        } else {
            M.ttab = tables_host[tt];
            M.trows = table_rows_host[tt];
        }
    }
    if (st == MPQE_OK && desc_bytes < rm_desc_size(num_formulas)) st = MPQE_ERR_WORKSPACE;
    if (st == MPQE_OK &&
        hipMemcpyAsync(desc, image, (size_t)num_formulas * sizeof(RgcnMixDesc), hipMemcpyHostToDevice, as_stream(stream)) !=
            hipSuccess)
        st = MPQE_ERR_LAUNCH;
    // (the copy reads pageable memory: it has left `image` when the call returns)
    delete[] image;
    return st;
}

static inline size_t rm_state_bytes(const TemplateDesc &d, int64_t Q, int64_t D) {
    return align_up((size_t)Q * (size_t)d.N * (size_t)D * 4, 256);
}
static inline size_t rm_out_bytes(int64_t Q, int64_t D) { return align_up((size_t)Q * (size_t)D * 4, 256); }
static inline bool rm_sizes_ok(int64_t Q, int64_t D) { return Q >= 0 && Q < ((int64_t)1 << 25) && D > 0 && D <= (1 << 20); }

extern "C" size_t mpqe_rgcn_mixed_workspace_bytes(int query_type, int64_t num_queries, int64_t dim) {
    if (query_type < 0 || query_type >= MPQE_Q_COUNT || !rm_sizes_ok(num_queries, dim)) return 0;
    return 2 * rm_state_bytes(kTemplates[query_type], num_queries, dim) + rm_out_bytes(num_queries, dim);
}

// Everything both entries check, then the encode launch. q_out == NULL: the workspace's own.
static int rm_encode(int query_type, int64_t num_formulas, const void *desc, size_t desc_bytes, const int64_t *node_map,
                     int64_t node_map_len, const float *mode_emb, const float *const *basis_host,
                     const float *const *root_host, const float *const *bias_host, int64_t num_relations, int passes,
                     int readout, int64_t dim, const int64_t *formula_of, const int64_t *anchors, int64_t num_queries,
                     void *workspace, size_t workspace_bytes, float *q_out, int32_t *err, RgcnMixArgs *out, void *stream) {
    if (query_type < 0 || query_type >= MPQE_Q_COUNT || num_queries < 0 || node_map_len < 0 || dim <= 0 || num_relations < 1)
        return MPQE_ERR_INVALID_ARG;
    if (!rm_formulas_ok(num_formulas)) return MPQE_ERR_INVALID_ARG;
    if (!desc || (uintptr_t)desc % 256 != 0 || !basis_host || !root_host) return MPQE_ERR_INVALID_ARG;
    if (readout != MPQE_READOUT_SUM && readout != MPQE_READOUT_MAX && readout != MPQE_READOUT_TM) return MPQE_ERR_UNSUPPORTED;
    if (passes < 1 || passes > RM_PASSES || dim % 4 != 0 || !rm_sizes_ok(num_queries, dim)) return MPQE_ERR_UNSUPPORTED;
    RgcnMixLayers W;
    memset(&W, 0, sizeof(W));
    for (int p = 0; p < passes; ++p) {
        if (!basis_host[p] || !root_host[p]) return MPQE_ERR_INVALID_ARG;
        if ((uintptr_t)basis_host[p] % 16 != 0 || (uintptr_t)root_host[p] % 16 != 0) return MPQE_ERR_UNSUPPORTED;
        W.basis[p] = basis_host[p];
        W.root[p] = root_host[p];
        W.bias[p] = bias_host ? bias_host[p] : nullptr;
    }
    if (desc_bytes < rm_desc_size(num_formulas)) return MPQE_ERR_WORKSPACE;
    if (num_queries == 0) return MPQE_OK;
    if (!mode_emb || !formula_of || !anchors || !workspace) return MPQE_ERR_INVALID_ARG;
    if ((uintptr_t)mode_emb % 16 != 0 || (uintptr_t)workspace % 16 != 0) return MPQE_ERR_UNSUPPORTED;
    if (workspace_bytes < mpqe_rgcn_mixed_workspace_bytes(query_type, num_queries, dim)) return MPQE_ERR_WORKSPACE;
    const TemplateDesc &d = kTemplates[query_type];
    RgcnMixArgs &G = *out;
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
    const size_t sb = rm_state_bytes(d, num_queries, dim);
    G.s0 = reinterpret_cast<float *>(wb);
    G.s1 = reinterpret_cast<float *>(wb + sb);
    G.q_out = q_out ? q_out : reinterpret_cast<float *>(wb + 2 * sb);
    G.err = err;
    const dim3 grid((unsigned)((num_queries + GT_BM - 1) / GT_BM * RM_STRETCHES));
    // the module path's own choice of load form (mpqe_rgcn_template_fwd with Din = Dout = dim, aligned operands)
    if (dim % GT_BN == 0)
        hipLaunchKernelGGL(rgcn_mixed_encode_kernel<LD_FAST>, grid, dim3(256), 0, as_stream(stream), G, W);
    else
        hipLaunchKernelGGL(rgcn_mixed_encode_kernel<LD_PRED>, grid, dim3(256), 0, as_stream(stream), G, W);
    return mpqe_launch_status();
}

extern "C" int mpqe_rgcn_embed_mixed(int query_type, int64_t num_formulas, const void *desc, size_t desc_bytes,
                                     const int64_t *node_map, int64_t node_map_len, const float *mode_emb,
                                     const float *const *basis_host, const float *const *root_host,
                                     const float *const *bias_host, int64_t num_relations, int passes, int readout,
                                     int64_t dim, const int64_t *formula_of, const int64_t *anchors, int64_t num_queries,
                                     void *workspace, size_t workspace_bytes, float *q_out, int32_t *err, void *stream) {
    if (num_queries > 0 && !q_out) return MPQE_ERR_INVALID_ARG;
    RgcnMixArgs G;
    return rm_encode(query_type, num_formulas, desc, desc_bytes, node_map, node_map_len, mode_emb, basis_host, root_host,
                     bias_host, num_relations, passes, readout, dim, formula_of, anchors, num_queries, workspace,
                     workspace_bytes, q_out, err, &G, stream);
}

extern "C" int mpqe_rgcn_fwd_mixed(int query_type, int64_t num_formulas, const void *desc, size_t desc_bytes,
                                   const int64_t *node_map, int64_t node_map_len, const float *mode_emb,
                                   const float *const *basis_host, const float *const *root_host,
                                   const float *const *bias_host, int64_t num_relations, int passes, int readout, int64_t dim,
                                   const int64_t *formula_of, const int64_t *anchors, int64_t num_queries, const int64_t *ids,
                                   const int64_t *qrow, int64_t n, float eps, void *workspace, size_t workspace_bytes,
                                   float *scores, int32_t *err, void *stream) {
    if (n < 0 || n >= ((int64_t)1 << 32)) return n < 0 ? MPQE_ERR_INVALID_ARG : MPQE_ERR_UNSUPPORTED;
    if (num_queries == 0 && n != 0) return MPQE_ERR_INVALID_ARG;
    if (n > 0 && (!ids || !qrow || !scores)) return MPQE_ERR_INVALID_ARG;
    RgcnMixArgs G;
    // (the score launch's own arguments are checked above: nothing is refused after the first launch)
    const int st = rm_encode(query_type, num_formulas, desc, desc_bytes, node_map, node_map_len, mode_emb, basis_host,
                             root_host, bias_host, num_relations, passes, readout, dim, formula_of, anchors, num_queries,
                             workspace, workspace_bytes, nullptr, err, &G, stream);
    if (st != MPQE_OK || num_queries == 0 || n == 0) return st;
    hipLaunchKernelGGL(rgcn_mixed_score_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, as_stream(stream), G,
                       reinterpret_cast<const long long *>(ids), reinterpret_cast<const long long *>(qrow), (long long)n, eps,
                       scores);
    return mpqe_launch_status();
}

// the mixed forward with states and the mixed backward
#include "rgcn_mixed_train.h"
