/* mpqe_amd.h -- C ABI of the MI355X-native MPQE R-GCN query-graph encoder.
 *
 * The reference (dfdazac/mpqe) is pure Python and has no FFI layer: its
 * boundary for this path is the nn.Module surface of mpqe/model.py plus the
 * torch_scatter / PyTorch Geometric calls it makes. Each entry point below
 * names the reference lines whose arithmetic it replaces. The Python mirror
 * (mpqe_amd/model.py, encoders.py, data_utils.py) binds these with ctypes.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless the name ends in _host;
 *   - floats are fp32, contiguous row-major; indices are int64 like the
 *     reference's LongTensors; sizes are int64_t;
 *   - the caller owns every buffer, including workspaces (query the size
 *     first); the library never allocates device memory and is re-entrant per
 *     stream. Host-side state, all behind one mutex: a cache of launch plans
 *     (pure functions of the descriptors, keyed by the caller's `desc`
 *     buffer). The library never reads the environment. The three
 *     mpqe_debug_* entry points at the end of this file are DIAGNOSTICS:
 *     process-global, off by default, to be set from one thread while no
 *     call is in flight; nothing in the data path depends on them;
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream); the fused
 *     step (mpqe_step_forward_backward) hands data from workgroup to workgroup
 *     INSIDE its launches and expects the GPU to itself: one process per GPU
 *     (several processes oversubscribing one GPU can exhaust its bounded spins
 *     -> MPQE_FLAG_INTERNAL, never a hang);
 *   - every function returns MPQE_OK or a negative MPQE_ERR_* code and never
 *     synchronises. Data-dependent faults (an index outside its table) cannot
 *     be seen from the host without a sync: kernels then skip the access and
 *     OR a MPQE_FLAG_* bit into the caller's `err` word (int32 in HBM, may be
 *     NULL); the host mirror raises IndexError from it like the reference's
 *     index_select would.
 */
#ifndef MPQE_AMD_H
#define MPQE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPQE_OK 0
#define MPQE_ERR_INVALID_ARG (-1)    /* null pointer, negative size, bad enum          */
#define MPQE_ERR_UNSUPPORTED (-2)    /* shape outside what the kernels cover           */
#define MPQE_ERR_WORKSPACE (-3)      /* workspace smaller than the *_workspace_bytes() */
#define MPQE_ERR_LAUNCH (-4)         /* hipGetLastError() != hipSuccess after launch   */

#define MPQE_FLAG_BAD_NODE_ID 1      /* entity id outside node_map / maps to -1        */
#define MPQE_FLAG_BAD_EDGE 2         /* edge endpoint outside [0, num_nodes)           */
#define MPQE_FLAG_BAD_RELATION 4     /* edge type outside [0, num_relations)           */
#define MPQE_FLAG_BAD_INDEX 8        /* scatter index outside [0, dim_size)            */
#define MPQE_FLAG_TOUCH_RETRY 32     /* the step could not build its own touch plan (MPQE_STEP_BUILD_TOUCH: the sort's
                                        workgroups were not all resident at once, e.g. on a shared GPU). Everything but
                                        the entity-table gradients is complete; those were NOT accumulated (dense: the
                                        step's zero fill stands; SPARSE_TABLES: the rows are untouched). Recover with
                                        mpqe_step_touch_build (MPQE_STEP_TOUCH_LIBRARY_SORT) + mpqe_step_table_rows.  */
#define MPQE_FLAG_INTERNAL 16        /* a hand-off between workgroups inside a launch did
                                        not arrive within its spin bound (library fault);
                                        bits 8.. say which (diagnostics: 0x100 a pre-pass
                                        vector, 0x200 the transposed copies, 0x400 a
                                        completion counter, 0x800 a vector op's inputs,
                                        0x2000 the touch plan's sort)                      */

/* query templates, reference data_utils.py:325-362 */
enum {
    MPQE_Q_1CHAIN = 0, MPQE_Q_2CHAIN = 1, MPQE_Q_3CHAIN = 2, MPQE_Q_2INTER = 3,
    MPQE_Q_3INTER = 4, MPQE_Q_3INTER_CHAIN = 5, MPQE_Q_3CHAIN_INTER = 6, MPQE_Q_COUNT = 7
};
enum { MPQE_READOUT_SUM = 0, MPQE_READOUT_MAX = 1, MPQE_READOUT_TM = 2,
       MPQE_READOUT_CALLER = 3 /* fused step only: the readout is the caller's (MPQE_STEP_PHASE_*) */,
       /* fused step only: the reference's learned readouts, Linear(in, dim) - ReLU - Linear(dim, dim) per row, then a
        * reduction over each graph's rows (mpqe_step_params_t.readout_*): MLP (model.py:497-515; in = dim, a row per node),
        * TARGETMLP (model.py:518-553; in = 2 dim, a row [target | node] per non-target node), CONCAT (model.py:441-446;
        * in = num_layers dim, a node's states after every layer side by side -- every batch runs num_layers passes).
        * They ride on the chain form when it applies (dim 64 / 128 / 256, at most 3 passes per batch, two free layer
        * slots): their Linear layers are two more levels of every graph block's programme; otherwise the level form (one
        * launch per level + dense-layer launches) */
       MPQE_READOUT_MLP = 4, MPQE_READOUT_TARGETMLP = 5, MPQE_READOUT_CONCAT = 6 };
enum { MPQE_SCATTER_ADD = 0, MPQE_SCATTER_MAX = 1, MPQE_SCATTER_MEAN = 2 };
#define MPQE_MAX_TEMPLATE_EDGES 3
#define MPQE_MAX_TEMPLATE_NODES 4

const char *mpqe_status_string(int status);
/* 5: MPQE_FLAG_TOUCH_RETRY, MPQE_STEP_TOUCH_LIBRARY_SORT, mpqe_step_table_rows (a failed in-step touch plan is recovered, not
 * fatal). 4: mpqe_step_params_t / mpqe_step_grads_t carry the learned readouts' Linear layers (readout_*); mpqe_step_states_layout,
 * MPQE_READOUT_CALLER and the MPQE_STEP_PHASE_* values of `backward`. 3: mpqe_linear_*, mpqe_debug_option, touch = OUT. */
int mpqe_abi_version(void);

/* Static shape of one query template (host side, no GPU needed).
 * reference: RGCNQueryDataset.query_edge_indices / query_diameters /
 * query_edge_label_idx / variable_node_idx, data_utils.py:325-362. */
typedef struct {
    int32_t num_anchors, num_vars, num_nodes, num_edges, diameter;
    int32_t src[MPQE_MAX_TEMPLATE_EDGES];      /* edge source row inside a graph     */
    int32_t dst[MPQE_MAX_TEMPLATE_EDGES];      /* edge destination row               */
    int32_t rel_label[MPQE_MAX_TEMPLATE_EDGES];/* index into Formula.get_rels()      */
    int32_t var_node[MPQE_MAX_TEMPLATE_NODES]; /* index into Formula.get_nodes()     */
} mpqe_template_t;
int mpqe_template_info(int query_type, mpqe_template_t *out_host);

/* ---- (a1) collation ------------------------------------------------------------------
 * reference: RGCNQueryDataset.get_query_graph data_utils.py:394-405 and PyG
 * Batch.from_data_list: B replicas of one template.
 *   edge_index[0, b*E+e] = src[e] + b*N     edge_index[1, b*E+e] = dst[e] + b*N
 *   edge_type[b*E+e] = edge_type_host[e]    batch[b*N+n] = b                        */
int mpqe_collate_template(int query_type, int64_t batch_size,
                          const int64_t *edge_type_host /*[E]*/,
                          int64_t *edge_index /*[2, B*E]*/, int64_t *edge_type /*[B*E]*/,
                          int64_t *batch /*[B*N]*/, void *stream);

/* ---- (a2, a3) entity embedding gather + L2 normalise -------------------------------------
 * reference: DirectEncoder.forward encoders.py:40-43 with the features closure
 * data_utils.py:35 (row = node_map[id]; v = table[row]; y = v / ||v||_2, no eps), written
 * where RGCNEncoderDecoder.forward puts it (model.py:418-420):
 *   out[i*out_row_stride + 0..dim) = y_i.   inv_norm[i] = 1/||v_i|| (optional, for bwd).
 * node_map == NULL means ids are table rows already (identity map).                        */
int mpqe_embed_l2norm_fwd(const float *table, int64_t table_rows, int64_t dim,
                          const int64_t *node_map, int64_t node_map_len,
                          const int64_t *ids, int64_t n,
                          float *out, int64_t out_row_stride, float *inv_norm /*[n] or NULL*/,
                          int32_t *err, void *stream);
/* grad_table[row_i] += (g_i - y_i (y_i . g_i)) / ||v_i||   (fp32 atomics on duplicates) */
int mpqe_embed_l2norm_bwd(const float *grad_out, int64_t grad_row_stride,
                          const float *table, int64_t table_rows, int64_t dim,
                          const int64_t *node_map, int64_t node_map_len,
                          const int64_t *ids, int64_t n,
                          float *grad_table /*[table_rows, dim], accumulated into*/,
                          int32_t *err, void *stream);
/* variable rows: out[(b*N + A + k)*dim ..] = mode_emb[var_ids[k]] for every b
 * reference: model.py:421. */
int mpqe_var_rows_fwd(const float *mode_emb, int64_t num_modes, int64_t dim,
                      const int64_t *var_ids /*[V]*/, int64_t num_vars,
                      int64_t batch_size, int64_t num_nodes, int64_t num_anchors,
                      float *x /*[B*N, dim]*/, int32_t *err, void *stream);
/* grad_mode_emb[var_ids[k]] += sum_b grad_x[(b*N + A + k)] (deterministic order) */
int mpqe_var_rows_bwd(const float *grad_x, int64_t num_modes, int64_t dim,
                      const int64_t *var_ids, int64_t num_vars,
                      int64_t batch_size, int64_t num_nodes, int64_t num_anchors,
                      float *grad_mode_emb, int32_t *err, void *stream);

/* ---- (a4) R-GCN layer -------------------------------------------------------------------
 * reference: RGCNConv.forward/message/update model.py:269-305 with PyG propagate +
 * torch_scatter.scatter_add ('add' aggregation, edge_norm None):
 *   out[i] = sum_{e: dst_e = i} x[src_e] . basis[type_e]  +  x[i] . root  +  bias
 * relu != 0 additionally applies the F.relu the caller puts after all but the last layer
 * (model.py:437).
 *
 * TEMPLATE form: the batch is B replicas of one template (row = b*N + n). The neighbour sum
 * runs inside the MFMA K loop: for node slot n with in-edges e1..ek the tile computes
 * [x[:,src_e1] | ... | x[:,n]] . [basis[r_e1]; ...; root], so nothing is scattered and no
 * [B*E, D, D] weight copy (model.py:292-293) exists.                                        */
int mpqe_rgcn_template_fwd(int query_type, int64_t batch_size,
                           const int64_t *edge_type_host /*[E] relation id per template edge*/,
                           const float *x /*[B*N, dim_in]*/,
                           const float *basis /*[R, dim_in, dim_out]*/, int64_t num_relations,
                           const float *root /*[dim_in, dim_out]*/, const float *bias /*[dim_out] or NULL*/,
                           int64_t dim_in, int64_t dim_out, int relu,
                           float *out /*[B*N, dim_out]*/, void *stream);
size_t mpqe_rgcn_template_bwd_workspace_bytes(int query_type, int64_t batch_size,
                                              int64_t dim_in, int64_t dim_out);
/* workspace (needed unless grad_basis, grad_root and grad_bias are all NULL): 16-byte aligned, any contents; too small
 * (MPQE_ERR_WORKSPACE) or misaligned (MPQE_ERR_INVALID_ARG) is refused before anything is queued, grad_x included. */
/* grad_out is d loss / d out (post-ReLU when relu != 0; `out` is then needed for the mask).
 * grad_x is overwritten; grad_basis / grad_root / grad_bias are ACCUMULATED into (dense, like
 * the reference's autograd). Any of the three may be NULL to skip it. Deterministic.        */
int mpqe_rgcn_template_bwd(int query_type, int64_t batch_size, const int64_t *edge_type_host,
                           const float *x, const float *out, const float *grad_out,
                           const float *basis, int64_t num_relations, const float *root,
                           int64_t dim_in, int64_t dim_out, int relu,
                           float *grad_x, float *grad_basis, float *grad_root, float *grad_bias,
                           void *workspace, size_t workspace_bytes, void *stream);

/* GENERAL form: arbitrary edge_index / edge_type (duplicates, self loops, isolated nodes,
 * unused relations). A plan sorts the edges once per graph: by relation for the grouped
 * MFMA GEMM, by destination (forward) and by source (backward) for the segmented sums.    */
size_t mpqe_rgcn_plan_bytes(int64_t num_nodes, int64_t num_edges, int64_t num_relations);
size_t mpqe_rgcn_plan_workspace_bytes(int64_t num_nodes, int64_t num_edges, int64_t num_relations);
int mpqe_rgcn_plan_build(const int64_t *edge_index /*[2, E]*/, const int64_t *edge_type /*[E]*/,
                         int64_t num_nodes, int64_t num_edges, int64_t num_relations,
                         void *plan, size_t plan_bytes, void *workspace, size_t workspace_bytes,
                         int32_t *err, void *stream);
/* workspace (forward and backward): 16-byte aligned, MPQE_ERR_INVALID_ARG otherwise, before anything is queued (which
 * kernels run, and so the last bits of the results, never depend on where it lies); nothing is assumed of what it holds. */
size_t mpqe_rgcn_general_workspace_bytes(int64_t num_nodes, int64_t num_edges, int64_t num_relations,
                                         int64_t dim_in, int64_t dim_out, int backward);
/* relu_mask (may be NULL; needs relu, dim_out % 64 == 0): mpqe_rgcn_general_mask_bytes(num_nodes, dim_out) bytes, 8-byte
 * aligned; the forward leaves the ReLU mask of `out` there as bit words (bit c % 64 of word [node][c / 64] = out > 0) and
 * the backward, given the same buffer, masks with them and never reads `out` (its gathered reads of `out` rows were a
 * third of the backward kernels' row traffic).                                                            */
size_t mpqe_rgcn_general_mask_bytes(int64_t num_nodes, int64_t dim_out);
int mpqe_rgcn_general_fwd(const void *plan, int64_t num_nodes, int64_t num_edges, int64_t num_relations,
                          const float *x, const float *basis, const float *root, const float *bias,
                          int64_t dim_in, int64_t dim_out, int relu, float *out, uint64_t *relu_mask,
                          void *workspace, size_t workspace_bytes, void *stream);
/* The scatter-aggregate of the forward alone (the destination-sorted segmented sum): out[i] = act(bias + msg[E + i] +
 * sum over the edges into i, in edge order, of their message rows); msg [E + Nn, dim] in the plan's slot order, as the
 * gather-GEMM of mpqe_rgcn_general_fwd leaves its messages (an edge's row = its position in the relation-sorted order,
 * the self term of node i at row E + i). Algorithmic bytes: 4 dim (E + 2 Nn).                                    */
int mpqe_rgcn_general_aggregate(const void *plan, int64_t num_nodes, int64_t num_edges, int64_t num_relations,
                                const float *msg, const float *bias, int64_t dim, int relu, float *out, void *stream);
/* overwrite = 0: grad_basis / grad_root / grad_bias are ACCUMULATED into (the caller zero-fills them); 1: every one of
 * them is WRITTEN whole, once -- the gradient, or zeros for a relation without an edge -- so the caller neither fills
 * [R, dim_in, dim_out] with zeros nor pays a read-modify-write of it (33 MB each at the stress shape). grad_x is always
 * written.                                                                                              */
int mpqe_rgcn_general_bwd(const void *plan, int64_t num_nodes, int64_t num_edges, int64_t num_relations,
                          const float *x, const float *out /* may be NULL with relu_mask */,
                          const uint64_t *relu_mask /* the forward's, or NULL */, const float *grad_out,
                          const float *basis, const float *root,
                          int64_t dim_in, int64_t dim_out, int relu, int overwrite,
                          float *grad_x, float *grad_basis, float *grad_root, float *grad_bias,
                          void *workspace, size_t workspace_bytes, void *stream);

/* ---- dense layer (the MLP readouts' nn.Linear, model.py:497-553; Encoder's compress product, encoders.py:120-124) ----
 * y [rows, dim_out] = [relu]( (accumulate ? y : 0) + x [rows, dim_in] . W^T + bias ), W [dim_out, dim_in] as nn.Linear
 * stores it, with row stride ldw >= dim_in (a column block of a wider matrix: the compress matrix applied to one
 * neighbour block at a time, the products accumulated, so the reference's concatenation is never materialised).
 * x, y, grad_y, grad_x contiguous. Backward: y = the layer's post-activation output (read only when relu != 0);
 * grad_x is written; grad_W [dim_out, .] (row stride ldgw) and grad_bias are accumulated into, or written
 * (overwrite = 1). Fixed-order reductions (no float atomics).                                              */
int mpqe_linear_fwd(const float *x, int64_t rows, const float *W, int64_t ldw, const float *bias, int64_t dim_in,
                    int64_t dim_out, int relu, int accumulate, float *y, void *stream);
/* workspace (needed unless grad_W and grad_bias are both NULL): 16-byte aligned, any contents; too small
 * (MPQE_ERR_WORKSPACE) or misaligned (MPQE_ERR_INVALID_ARG) is refused before anything is queued, grad_x included. */
size_t mpqe_linear_bwd_workspace_bytes(int64_t rows, int64_t dim_in, int64_t dim_out);
int mpqe_linear_bwd(const float *x, int64_t rows, const float *W, int64_t ldw, const float *y, const float *grad_y,
                    int64_t dim_in, int64_t dim_out, int relu, int overwrite, float *grad_x, float *grad_W, int64_t ldgw,
                    float *grad_bias, void *workspace, size_t workspace_bytes, void *stream);

/* ---- (a5) readouts ----------------------------------------------------------------------
 * Regular form for template batches (batch_idx = b repeated N):
 *   SUM  reference sum_readout model.py:380-381   out[b] = sum_n h[b*N+n]
 *   MAX  reference max_readout model.py:383-385   out[b] = max_n h[b*N+n]; argmax[b,d] = lowest n
 *   TM   reference target_message_readout 387-398 out[b] = h[b*N + A]                        */
int mpqe_readout_fwd(int kind, const float *h, int64_t batch_size, int64_t num_nodes,
                     int64_t num_anchors, int64_t dim, float *out /*[B, dim]*/,
                     int32_t *argmax /*[B, dim], MAX only, may be NULL*/, void *stream);
int mpqe_readout_bwd(int kind, const float *grad_out /*[B, dim]*/, const int32_t *argmax,
                     int64_t batch_size, int64_t num_nodes, int64_t num_anchors, int64_t dim,
                     float *grad_h /*[B*N, dim], overwritten*/, void *stream);
/* torch_scatter.scatter_add / scatter_max / scatter_mean along dim 0 (reference call sites
 * model.py:351-355, 381, 384, 509, 547). index may come in any order.
 * out[i] = reduce_{j: index[j] = i} src[j]; empty rows are 0; arg = lowest j on ties, -1 empty.
 * add / mean accumulate with fp32 atomics (order-dependent last bits when rows collide).     */
size_t mpqe_scatter_workspace_bytes(int64_t n_src, int64_t dim_size);
int mpqe_scatter_fwd(int op, const float *src, const int64_t *index, int64_t n_src, int64_t dim,
                     int64_t dim_size, float *out /*[dim_size, dim]*/, int64_t *arg /*MAX only*/,
                     void *workspace, size_t workspace_bytes, int32_t *err, void *stream);
int mpqe_scatter_bwd(int op, const float *grad_out, const int64_t *index, const int64_t *arg,
                     int64_t n_src, int64_t dim, int64_t dim_size, float *grad_src,
                     void *workspace, size_t workspace_bytes, void *stream);

/* ---- (a9) LayerNorm + ReLU of the GraphSAGE-style Encoder ---------------------------------------
 * reference encoders.py:132-146 (unbiased std, eps added to the std) + the Encoder's ReLU (encoders.py:127-128):
 *   y = act(gamma * (x - mean) / (std + eps) + beta), per row of x [rows, dim]; stats [rows, 2] = {mean, 1/(std+eps)}.
 * bwd: grad_x overwritten; grad_gamma / grad_beta ACCUMULATED (fixed-order column sums).                */
int mpqe_layernorm_relu_fwd(const float *x, int64_t rows, int64_t dim, const float *gamma, const float *beta, float eps,
                            int relu, float *y, float *stats, void *stream);
size_t mpqe_layernorm_relu_bwd_workspace_bytes(int64_t rows, int64_t dim);
int mpqe_layernorm_relu_bwd(const float *grad_y, const float *x, const float *y, int64_t rows, int64_t dim,
                            const float *gamma, const float *stats, float eps, int relu, float *grad_x,
                            float *grad_gamma, float *grad_beta, void *workspace, size_t workspace_bytes, void *stream);

/* ---- (a6, a7) scoring and loss ------------------------------------------------------------
 * reference: F.cosine_similarity(q, t, dim=1) model.py:452, 458 (eps 1e-8 clamps each norm):
 *   scores[i] = q[qrow(i)] . t[i] / (max(||q||, eps) * max(||t||, eps))
 * q_row (may be NULL = identity) is the repeat_interleave(out, neg_lengths) map of model.py:456. */
int mpqe_cosine_fwd(const float *q, const int64_t *q_row, const float *t, int64_t n, int64_t dim,
                    float eps, float *scores, void *stream);
/* grad_q is ACCUMULATED into when q_row != NULL (several i share a row; fp32 atomics),
 * overwritten otherwise; grad_t overwritten. Either may be NULL.                          */
int mpqe_cosine_bwd(const float *grad_scores, const float *q, const int64_t *q_row, const float *t,
                    int64_t n, int64_t dim, float eps, float *grad_q, float *grad_t, void *stream);
/* reference margin_loss model.py:483-485: loss = mean(clamp(margin - (pos - neg), min=0)).
 * Deterministic single-block reduction. */
int mpqe_hinge_fwd(const float *pos, const float *neg, int64_t n, float margin, float *loss, void *stream);
int mpqe_hinge_bwd(const float *pos, const float *neg, int64_t n, float margin, const float *grad_loss /*[1]*/,
                   float *grad_pos, float *grad_neg, void *stream);

/* ---- answering a query: all rows of one mode's table ranked against Q query embeddings ----------------------
 * (the reference has no such call; the score is the one its model gives a candidate, model.py:452:)
 *   score(i, r) = cosine_similarity(q[i], table[r] / ||table[r]||, eps)
 * with the row normalisation of mpqe_embed_l2norm_fwd and the norm clamp of mpqe_cosine_fwd, formed as
 * ((q[i] . table[r]) * 1/||table[r]||) * 1/max(||q[i]||, eps) on the fp32 MFMA tile -- a function of q[i] and table[r] alone,
 * so rank, top-k and exclusions agree exactly. A zero table row scores 0; a NaN score ranks last (-inf). The [Q, N] score
 * matrix is never written to memory. Everything is in TABLE ROWS; the caller translates entity ids.
 * Total order: higher fp32 score first, the smaller row on equal scores.
 *   excl_offsets [Q+1], excl_rows [num_excluded]: CSR of the rows NOT eligible for query i, each list sorted ascending
 *             (repeats allowed; a descent ORs MPQE_FLAG_BAD_INDEX). Both NULL / num_excluded 0: every row is eligible.
 *   topk_rows, topk_scores [Q, k] (k > 0): the first min(k, eligible_i) eligible rows of query i in the total order,
 *             then -1 / -inf. k <= 128 (the per-query candidate lists live in LDS), MPQE_ERR_UNSUPPORTED above.
 *   rank [Q] (needs target_rows): 1 + the number of eligible rows other than the target that precede the target. The
 *             target itself is never excluded, listed or not (filtered evaluation lists every known answer).
 *   target_scores [Q] (needs target_rows; may be NULL): score(i, target_rows[i]).
 * A target or excluded row outside [0, table_rows) ORs MPQE_FLAG_BAD_INDEX into err and is not dereferenced: such a
 * target gives rank -1 / score NaN, such an excluded row excludes nothing; the other queries are unaffected.
 * Integer counters only (integer atomics), fixed-order merge: bit-identical run to run, and for any split of the
 * queries over calls. table_rows, num_queries <= 2^30, dim <= 2^20. num_queries == 0 is a no-op.             */
size_t mpqe_rank_workspace_bytes(int64_t num_queries, int64_t table_rows, int64_t dim, int k);
int mpqe_rank_entities(const float *q /*[Q, dim]*/, int64_t num_queries, const float *table /*[table_rows, dim], raw rows*/,
                       int64_t table_rows, int64_t dim, float eps, const int64_t *target_rows /*[Q] or NULL*/,
                       const int64_t *excl_offsets, const int64_t *excl_rows, int64_t num_excluded, int k /*0: no top-k*/,
                       int64_t *topk_rows, float *topk_scores, int64_t *rank, float *target_scores, void *workspace,
                       size_t workspace_bytes, int32_t *err, void *stream);
/* The same call with the score chosen (added under ABI 7: an entry only). score_kind 0: the cosine above --
 * mpqe_rank_entities is this call with 0. score_kind 1: score(i, r) = q[i] . table[r], the plain dot product the diagonal
 * path decoder gives a chain query (mpqe_gqe_fwd, programme int [27]): the pre-pass writes 1.0f for both factors, so the
 * score is the MFMA dot's own bits and eps is not read. Scores are then finite but unbounded and often negative; order,
 * ties, exclusions, rank and top-k are as above. Another score_kind: MPQE_ERR_INVALID_ARG. */
int mpqe_rank_entities_scored(const float *q, int64_t num_queries, const float *table, int64_t table_rows, int64_t dim,
                              float eps, int score_kind, const int64_t *target_rows, const int64_t *excl_offsets,
                              const int64_t *excl_rows, int64_t num_excluded, int k, int64_t *topk_rows, float *topk_scores,
                              int64_t *rank, float *target_scores, void *workspace, size_t workspace_bytes, int32_t *err,
                              void *stream);

/* Queries of ONE call ranked against DIFFERENT tables (csrc/rank_mixed.hip; added under ABI 7: entries only). Query i is
 * ranked against candidate set set_of_group[group_of[i]] of num_sets sets -- in an evaluation window the group is the
 * query's formula and the set the entities of the formula's target mode.
 *
 * mpqe_rank_mixed_desc_build writes the sets to `desc` (device memory, 256-byte aligned, mpqe_rank_mixed_desc_bytes: exact,
 * a byte less is MPQE_ERR_WORKSPACE; 0: a count out of range). Host arrays, per set: tables_host the device address of raw
 * rows [rows_host[s], dim] (16-byte aligned, MPQE_ERR_UNSUPPORTED otherwise), rows_host >= 1, kinds_host the score kind of
 * mpqe_rank_entities_scored (0 cosine, 1 dot), valid_host (the array or an entry may be NULL: every row valid) the device
 * address of ceil(rows / 32) uint32 words, bit r clear = row r is no entity and never eligible. set_of_group_host
 * [num_groups] in [0, num_sets). 1 <= num_sets <= 256, 1 <= num_groups <= 2^20, the rows of all sets <= 2^30. Everything
 * is checked before anything is written. The block holds addresses and sizes only: the caller keeps it between calls and
 * a ranking call does no host work per set or per group.
 *
 * mpqe_rank_entities_mixed: num_sets, num_groups, max_rows (the widest set) and total_rows (all sets') are the block's own
 * (a call that names other values flags MPQE_FLAG_BAD_INDEX and ranks nothing). group_of [Q] int64 on the device.
 * target_rows [Q] or NULL: rows of the query's own set. excl_bits or NULL: [Q, excl_stride_words] int32 words, the layout
 * of the KG index's answer bitmaps; bit r of row i set = row r is not eligible for query i; bits at or beyond the rows of
 * the query's set, and words the stride does not cover, are not read as exclusions. topk_rows, topk_scores, rank,
 * target_scores: the layouts and meanings of mpqe_rank_entities. Workspace: 256-byte aligned,
 * mpqe_rank_mixed_workspace_bytes (exact; 0: out of range); its contents on entry do not matter.
 * Rank, every top-k row and score and the target score of query i equal BIT FOR BIT what mpqe_rank_entities_scored returns
 * when the queries of i's set are handed to it alone with the set's score kind and, as exclusion list, the set's rows
 * whose excl_bits bit is set or whose valid bit is clear. Total order, the target never being excluded from its rank, NaN
 * last and integer counters as there. The outputs of a query depend neither on the order of the queries (a permutation
 * of the queries permutes the outputs) nor on how they are split over calls.
 * Launches: a plan (stable sort of the queries by set, blocks of 64 queries of one set: at most Q / 64 + num_sets, the
 * grids are sized to that bound on the host), then the pre-pass, the targets, the tiles and the merge of
 * mpqe_rank_entities, each reading its queries through the permutation and its table through the block's set. Exclusion
 * is a bit test in the tile kernel (two words per query and 64-row tile).
 * A group_of[i] outside [0, num_groups) or a target row outside its set ORs MPQE_FLAG_BAD_INDEX: rank -1, score NaN (a bad
 * group: also a top-k of -1 / -inf); the other queries are unaffected and nothing is read or written out of bounds.
 * num_queries == 0: MPQE_OK, no launch. k > 128: MPQE_ERR_UNSUPPORTED. */
size_t mpqe_rank_mixed_desc_bytes(int64_t num_sets, int64_t num_groups);
int mpqe_rank_mixed_desc_build(const float *const *tables_host, const int64_t *rows_host, const int32_t *kinds_host,
                               const uint32_t *const *valid_host, int64_t num_sets, const int32_t *set_of_group_host,
                               int64_t num_groups, void *desc, size_t desc_bytes, void *stream);
size_t mpqe_rank_mixed_workspace_bytes(int64_t num_queries, int64_t num_sets, int64_t max_rows, int64_t total_rows,
                                       int64_t dim, int k);
int mpqe_rank_entities_mixed(const float *q /*[Q, dim]*/, int64_t num_queries, int64_t dim, float eps, const void *desc,
                             size_t desc_bytes, int64_t num_sets, int64_t num_groups, int64_t max_rows, int64_t total_rows,
                             const int64_t *group_of, const int64_t *target_rows, const int32_t *excl_bits,
                             int64_t excl_stride_words, int k, int64_t *topk_rows, float *topk_scores, int64_t *rank,
                             float *target_scores, void *workspace, size_t workspace_bytes, int32_t *err, void *stream);

/* ---- fused training step -------------------------------------------------------------------
 * Forward + backward of RGCNEncoderDecoder.margin_loss (reference model.py:464-494) for ALL the
 * formula batches of one training step (reference train_helpers.py:76-120 draws 11 after
 * burn-in), each with explicit positive and negative targets, in 2 - 3 launches (dim 64 / 128 / 256: the
 * graph-block chain form; ~15 launches in the level form, MPQE_STEP_NO_CHAIN or other dims):
 *     loss[0] = sum_b weight_b * mean_i clamp(margin - (pos_bi - neg_bi), 0);  loss[1+b] = that mean
 * Gradients of every parameter are ACCUMULATED into `grads` (dense, like the reference's
 * autograd). Readouts: sum / max / mp(TM). The query embedding is computed once per batch and
 * scored against both targets (the reference encodes twice; same maths).
 * Descriptors are HOST structs; every pointer inside them is a device pointer.               */
#define MPQE_STEP_MAX_BATCHES 16
#define MPQE_STEP_MAX_LAYERS 8
#define MPQE_STEP_MAX_MODES 16
/* mpqe_step_params_t.flags -- speed switches; loss, scores and gradients are the same either way:
 * NO_PRUNE  also compute node states that cannot reach the readout (the reference computes all of them;
 *           with the TM readout only the target row is read, model.py:391-398, so e.g. 9 of the 21
 *           node updates of a 3-chain feed nothing and get an exactly-zero gradient). Default: skip them.
 * NO_CHAIN  one launch per message-passing level instead of the graph-block chain kernels.      */
#define MPQE_STEP_NO_PRUNE 1
#define MPQE_STEP_NO_CHAIN 2
/* ZERO_GRADS  the call zero-fills every buffer of `grads` before accumulating into it (one launch shared
 *             with the step's other prologue work, instead of a memset per buffer by the caller).    */
#define MPQE_STEP_ZERO_GRADS 4
/* NO_KSPLIT   dim 128 only: the chain kernel's waves each own 32 columns and the whole K range (the first form)
 *             instead of 64 columns and half of K.                                                     */
#define MPQE_STEP_NO_KSPLIT 8
/* EIGHT_WAVES dim 128 only, experimental: chain workgroups of eight waves (a wave of each K half on every SIMD, 32
 *             columns each) instead of four. Same results; measured 1 % slower on the AIFB mix.  */
#define MPQE_STEP_EIGHT_WAVES 16
/* NO_UNIFORM  chain form: treat every node state as per-graph rows. Default: node states no anchor has reached yet
 *             are ONE vector per batch (the variable rows of x0 are the same mode_embeddings row for every graph of
 *             a batch, reference model.py:421), so their updates are matrix-VECTOR products done once per batch by a
 *             pre-pass, their backward runs on column sums, and their weight gradients are rank-1 updates -- the
 *             AIFB mix keeps 34 of its 66 live [B, D] x [D, D] products per direction.                       */
#define MPQE_STEP_NO_UNIFORM 32
/* SPARSE_TABLES  (with a touch plan) the entity-table gradients are delivered ROW-SPARSE: the rows the step's ids
 *             touched are written (not accumulated) into the dense `grads->tables` buffers and every other row is
 *             left as it is -- no zero fill and no pass over tables of 10^5 .. 10^6 rows per step. For consumers that
 *             read only the touched rows: mpqe_adam_rows_step, the row exchange of the data-parallel path.      */
#define MPQE_STEP_SPARSE_TABLES 64
/* MERGE_TAIL / SPLIT_TAIL  (chain form) where the weight-gradient tiles and the backward post-pass run. Merged: as
 *             workgroups of the chain launch itself, queued behind the chain workgroups and started per batch as soon
 *             as that batch's chain workgroups have published their rows (two launches per step: chain, reduction).
 *             Split: as a launch of their own behind the chain launch (three launches). Same results either way.
 *             Default: merged while the step has at most 9/8 x 256 chain workgroups (16 query graphs each) -- there
 *             it is 4 .. 12 % faster --, split beyond (the AIFB step of 11 x 512 graphs: merged is 4 % slower).
 *             MERGE_TAIL forces the merged form, SPLIT_TAIL the split one.                                    */
#define MPQE_STEP_MERGE_TAIL 128
#define MPQE_STEP_SPLIT_TAIL 256
/* BUILD_TOUCH  (chain form, backward) the step builds the touch plan of the ids it is called with ITSELF, by workgroups
 *             that lead its first launch and run beside the forward / backward chains (step_touch.h): `touch` is then an
 *             OUTPUT buffer (mpqe_step_touch_bytes; valid once the call has run: mpqe_adam_rows_step and the row exchange
 *             read its keys), and a step with fresh ids costs no more than a replayed one -- nothing id-dependent is left
 *             for collation time (the reference resolves ids and accumulates embedding gradients inside forward /
 *             backward: encoders.py:40-43, data_utils.py:35). The level form has no use for a plan and leaves the buffer
 *             alone. Steps of more than 524 288 looked-up ids, or split over stream lanes, return MPQE_ERR_UNSUPPORTED:
 *             build the plan with mpqe_step_touch_build instead.                                              */
/*             The plan buffer must be ZERO-FILLED once, before its first use as an output: a build that gives up
 *             (MPQE_FLAG_TOUCH_RETRY) leaves it as it was, and the step's last launch reads plan entries before it knows. */
#define MPQE_STEP_BUILD_TOUCH 512
/* ADD_STATE_GRADS  (MPQE_READOUT_CALLER, PHASE_FROM_STATES) the caller's readout read the states of EVERY level 1 .. L_b
 *             (the reference's `concat` readout, model.py:441-446) and has written its d loss / d state into every row of
 *             those gradient levels, not only the final one: the backward adds the gradient it propagates to them.  */
#define MPQE_STEP_ADD_STATE_GRADS 1024
/* TOUCH_LIBRARY_SORT  (mpqe_step_touch_build only) build the plan with the library's multi-launch radix sort instead of
 *             the one-launch sort whose workgroups synchronise among themselves: slower, and independent of how many
 *             workgroups the device can hold at once -- the recovery path behind MPQE_FLAG_TOUCH_RETRY.          */
#define MPQE_STEP_TOUCH_LIBRARY_SORT 2048

typedef struct {
    int32_t query_type;        /* MPQE_Q_*                                                     */
    int32_t num_passes;        /* message-passing passes: diameter if adaptive else num_layers */
    int32_t batch_size;        /* B: query graphs of this formula                              */
    int32_t target_mode;       /* entity-table index of the targets / negatives                */
    int64_t edge_type[MPQE_MAX_TEMPLATE_EDGES];  /* relation id per template edge              */
    int64_t var_ids[MPQE_MAX_TEMPLATE_NODES - 1];/* mode id per variable node                  */
    int32_t anchor_mode[MPQE_MAX_TEMPLATE_EDGES];/* entity-table index per anchor slot         */
    float weight;              /* weight of this batch's loss in the step loss                 */
} mpqe_step_batch_t;

typedef struct {
    int32_t dim, num_layers, num_relations, num_modes;
    int32_t readout;           /* MPQE_READOUT_*                                               */
    int32_t flags;             /* MPQE_STEP_* bits below; 0 = everything on                    */
    const float *tables[MPQE_STEP_MAX_MODES];    /* per-mode entity table [rows, dim]          */
    int64_t table_rows[MPQE_STEP_MAX_MODES];
    const int64_t *node_map;   /* global entity id -> row of its mode's table (-1: none)       */
    int64_t node_map_len;
    const float *mode_emb;     /* [num_modes, dim]                                             */
    const float *basis[MPQE_STEP_MAX_LAYERS];    /* layers[i].basis [R, dim, dim]; shared      */
    const float *root[MPQE_STEP_MAX_LAYERS];     /* layers repeat the same pointers            */
    const float *bias[MPQE_STEP_MAX_LAYERS];
    /* learned readouts (MPQE_READOUT_MLP / _TARGETMLP / _CONCAT): the two Linear layers as nn.Linear stores them
     * (weight [out, in] row-major, bias [out]); readout_scatter = MPQE_SCATTER_* of the reduction (the reference's
     * --scatter_op); readout_weight_decay: model.py:486-490, loss += weight_decay * (sum of the four parameters'
     * 2-norms) per margin_loss call, i.e. times the sum of the batch weights (0 = off). dim % 4 == 0; chain form: 16-byte
     * aligned parameters.                                                                                             */
    const float *readout_w0, *readout_b0, *readout_w2, *readout_b2;
    int32_t readout_scatter;
    float readout_weight_decay;
} mpqe_step_params_t;

/* Alignment of the step's operands (mpqe_step_params_t, mpqe_step_grads_t, the ids, loss and scores). The level form
 * takes any pointer aligned for its element type (4 bytes for the float operands): where a parameter, a table or a
 * gradient buffer is not on a 16-byte boundary, or dim % 4 != 0, its kernels run their scalar forms. The chain form (dim
 * 64 / 128 / 256) takes 16-byte aligned parameters and gradient buffers: a step whose PARAMETERS are not is planned as a
 * level-form step (the size queries see them); GRADIENT buffers that are not (mode_emb, basis, root, bias, readout_*; and
 * tables with a touch plan) make the call return MPQE_ERR_INVALID_ARG before anything is queued -- the form was chosen, and
 * workspace and descriptors sized, before the gradients were known. MPQE_STEP_NO_CHAIN asks for the level form. Entity-table
 * gradients added by atomics (touch = NULL), the ids, loss and the scores are scalar accesses in both forms.            */
typedef struct {
    float *tables[MPQE_STEP_MAX_MODES];          /* NULL = not wanted                          */
    float *mode_emb;
    float *basis[MPQE_STEP_MAX_LAYERS];
    float *root[MPQE_STEP_MAX_LAYERS];
    float *bias[MPQE_STEP_MAX_LAYERS];
    float *readout_w0, *readout_b0, *readout_w2, *readout_b2;      /* learned readouts                  */
} mpqe_step_grads_t;

/* Stream lanes (optional). At the reference's batch size every launch of the step is short enough that
 * its fixed cost (~8 us: dispatch, descriptor + first-tile latency, drain) dominates, and one step is a
 * chain of ~13 dependent launches. With lanes, lane l runs the whole chain (assemble -> message-passing
 * levels -> score -> levels back) of batches [batch_begin[l], batch_begin[l+1]) on its own stream; lane 0
 * is `stream`. The lanes fork after the descriptor upload and join before the weight-gradient launch (chain
 * form: every lane also launches the weight gradients of its own batches, the lanes join before the reduction).
 * The caller owns the streams and events (no allocation, no synchronisation in the library).          */
#define MPQE_STEP_MAX_LANES 4
typedef struct {
    int32_t num_lanes;                              /* 1 .. MPQE_STEP_MAX_LANES                      */
    int32_t batch_begin[MPQE_STEP_MAX_LANES + 1];   /* ascending, [0] = 0, [num_lanes] = num_batches */
    void *aux_stream[MPQE_STEP_MAX_LANES];          /* hipStream_t of lanes 1.. ([0] unused)         */
    void *fork_event;                               /* hipEvent_t                                    */
    void *join_event[MPQE_STEP_MAX_LANES];          /* hipEvent_t of lanes 1.. ([0] unused)          */
} mpqe_step_lanes_t;

size_t mpqe_step_workspace_bytes(const mpqe_step_params_t *params_host, const mpqe_step_batch_t *batches_host,
                                 int num_batches, const mpqe_step_lanes_t *lanes /* NULL = one lane */);
/* The kernels read a small descriptor table (templates, relations, offsets, reduction groups). It
 * lives in a caller-owned device buffer `desc` (256-byte aligned): with upload_desc != 0 the call
 * first writes it (by kernel arguments, no host memory is read asynchronously); a packed step
 * that is run again unchanged passes upload_desc = 0 and re-uses it -- building it is part of
 * collation, like the reference's collate_fn building edge_index / edge_type.                  */
size_t mpqe_step_desc_bytes(const mpqe_step_params_t *params_host, const mpqe_step_batch_t *batches_host,
                            int num_batches, const mpqe_step_lanes_t *lanes /* the split the step will run with */);
/* Entity-table gradients without float atomics ("touch plan"). The reference's autograd scatters the gradient rows
 * of the looked-up entities into the dense tables with index_add (deterministic on the CPU). Which looked-up ids share
 * a table row is a function of the ids alone, so it is found once per packed step, at collation time:
 * mpqe_step_touch_build gathers (table, row) keys through node_map and sorts them (stable) into `touch`, a caller-owned
 * device buffer (256-byte aligned, mpqe_step_touch_bytes; scratch: mpqe_step_touch_workspace_bytes, free after the
 * call has run). Handed to mpqe_step_forward_backward (chain form), the step stores one gradient row per looked-up id
 * and adds the rows of each table row in that fixed order: bit-reproducible, and no atomic traffic. touch = NULL keeps
 * the fp32-atomic form (results equal up to the order of the additions). The ids must be the ones the step is run with. */
size_t mpqe_step_touch_bytes(const mpqe_step_params_t *params_host, const mpqe_step_batch_t *batches_host,
                             int num_batches);
size_t mpqe_step_touch_workspace_bytes(const mpqe_step_params_t *params_host, const mpqe_step_batch_t *batches_host,
                                       int num_batches);
int64_t mpqe_step_touch_entries(const mpqe_step_batch_t *batches_host, int num_batches);   /* looked-up ids of a step */
int mpqe_step_touch_build(const mpqe_step_params_t *params_host, const mpqe_step_batch_t *batches_host, int num_batches,
                          const int64_t *anchor_ids, const int64_t *targets, const int64_t *negs, void *touch,
                          size_t touch_bytes, void *workspace, size_t workspace_bytes, void *stream);
/* anchor_ids: per batch b a block of [A_b, B_b] ids (slot-major), blocks concatenated in batch
 * order; targets / negs: [sum_b B_b]. backward = 0 stops after the loss (grads may be NULL).
 * scores_pos / scores_neg: [sum_b B_b] or NULL. workspace must be 256-byte aligned.
 * lanes (may be NULL = one lane): see mpqe_step_lanes_t.
 * events (may be NULL): hipEvent_t handles recorded in pairs around single launches on the stream of the
 * launch, in this order: for level 0..Lmax-1, for each lane that has the level: layer forward; for level
 * Lmax-1..0, for each such lane: backward-x; then the weight-gradient launch. When the graph-block chain
 * kernel runs (dim 64 / 128 / 256, MPQE_STEP_NO_CHAIN clear, every batch at most 5 passes) the order is: the chain
 * launch (ONE launch on the caller's stream whatever `lanes` says: prologue, assemble, levels forward, scores, levels
 * backward; forward-only steps record this pair alone), then the weight-gradient launch (with the merged tail its
 * tiles ride in the chain launch: the pair is still recorded, round nothing); in both forms last the step's
 * reduction launch. Fewer are filled as far as they go.
 * For roofline accounting only.                                                                     */
/* readout = MPQE_READOUT_CALLER: the step in THREE calls around a readout the caller computes itself -- the learned
 * readouts of the reference (MLPReadout / TargetMLPReadout, model.py:497-553), whose Linear layers are the caller's
 * (mpqe_linear_fwd / bwd); everything else of the step stays in the library. `backward` then names the call; the
 * level form runs (node states in HBM, every state live), one lane. Same params / batches / ids / desc / workspace in all
 * calls; upload_desc as usual in the first, 0 afterwards. (readout CALLER with backward 0 / 1, or a phase with another
 * readout: MPQE_ERR_INVALID_ARG.)
 *   PHASE_STATES       zero fill (MPQE_STEP_ZERO_GRADS), gather, every level forward. Afterwards the node states of
 *                      level p are rows [rows_total, dim] at workspace + states_offset + 4 * p * level_stride
 *                      (mpqe_step_states_layout); batch b's graphs own rows row_offset[b] + g * N_b + n, and its final
 *                      states are those of level num_passes_b.
 *   PHASE_SCORES       the caller has written the query embeddings [graphs_total, dim] (batch order) at workspace +
 *                      queries_offset: cosine scores against the targets / negatives, hinge terms, d loss / d embedding
 *                      to workspace + query_grads_offset, the targets' / negatives' entity-table gradients into grads.
 *                      scores_pos / scores_neg are written.
 *   PHASE_FROM_STATES  the caller has put d loss / d (final state) into the same rows of the gradient levels
 *                      (workspace + grads_offset + ...) -- every row of a batch's final level --: levels backward,
 *                      weight / bias / mode-vector gradients, the anchors' entity-table gradients, the reduction;
 *                      `loss` is written.
 *   PHASE_SCORES_ONLY  PHASE_SCORES without gradients, and `loss` written: the forward-only step (grads may be NULL). */
#define MPQE_STEP_PHASE_STATES 2
#define MPQE_STEP_PHASE_SCORES 3
#define MPQE_STEP_PHASE_FROM_STATES 4
#define MPQE_STEP_PHASE_SCORES_ONLY 5
int mpqe_step_states_layout(const mpqe_step_params_t *params_host, const mpqe_step_batch_t *batches_host,
                            int num_batches, const mpqe_step_lanes_t *lanes, int64_t *states_offset /* bytes */,
                            int64_t *grads_offset /* bytes */, int64_t *level_stride /* floats */,
                            int64_t *row_offset /* [num_batches + 1], rows */, int64_t *queries_offset /* bytes */,
                            int64_t *query_grads_offset /* bytes */);
int mpqe_step_forward_backward(const mpqe_step_params_t *params_host, const mpqe_step_batch_t *batches_host,
                               int num_batches, const int64_t *anchor_ids, const int64_t *targets,
                               const int64_t *negs, float margin, const mpqe_step_grads_t *grads_host,
                               int backward, float *loss /*[1 + num_batches]*/, float *scores_pos,
                               float *scores_neg, void *desc, size_t desc_bytes, int upload_desc,
                               void *workspace, size_t workspace_bytes, int32_t *err,
                               const mpqe_step_lanes_t *lanes, void *const *events, int num_events,
                               void *touch /* mpqe_step_touch_build's buffer (read), the plan buffer to fill (MPQE_STEP_BUILD_TOUCH), or
                                              NULL */, void *stream);

/* The same call with per-call extras (extra = NULL: exactly mpqe_step_forward_backward). For the host mirror's drop-in
 * entry points -- RGCNEncoderDecoder.margin_loss / .forward (reference model.py:400-494) routed through the fused step:
 *   batch_weight[i]  a DEVICE scalar (or NULL = 1): batch i's loss weight is batches_host[i].weight * *batch_weight[i],
 *                    read when the step runs. `loss = l_0 + w_1 * l_1 + ...; loss.backward()` (reference
 *                    train_helpers.py:81-119) hands every margin_loss node its upstream gradient as a 0-dim device tensor:
 *                    the backward of ALL nodes is then ONE step whose weights are those tensors, with no device-to-host read.
 *                    The weights scale the gradients (and the readout regulariser's, model.py:486-490); loss[0] is formed
 *                    with the host weights alone. A launch of one workgroup writes them into the resident descriptor table
 *                    in front of the step's launches (a later call without extras writes the host weights back).
 *   query_out        [sum_b B_b, dim] or NULL: the query embeddings (the readout's output rows, model.py:447-449) in batch
 *                    order -- what the evaluation form scores against ragged negative lists (model.py:454-460,
 *                    mpqe_cosine_fwd with q_row). Chain form only (MPQE_ERR_UNSUPPORTED otherwise).
 *   notify           two 32-bit words the DEVICE can write and the host can read without a call (pinned host memory), or
 *                    NULL: the workgroup that forms the loss (behind every launch and workgroup of the call that reads the
 *                    ids) stores notify[1] = the error word as it
 *                    stands, then notify[0] = notify_value. Once the host reads notify_value there, every launch of the call
 *                    that reads anchor_ids / targets / negs has run (the id arrays may be refilled), and notify[1] tells
 *                    whether a bad id was met -- the reference raises IndexError inside forward (encoders.py:40-43); a host
 *                    mirror that must not synchronise per call polls this word instead.
 *   xcd_shift        0 .. 7: a FORWARD-ONLY step in the chain form places its workgroups `xcd_shift` XCDs further round the
 *                    chip (a batch's graph blocks are dealt to one XCD per 32, so that its matrices stay in one L2; workgroup
 *                    b of a launch runs on XCD b % 8). Forward-only steps of SEVERAL packed steps issued on different streams
 *                    at once (each with a workspace of its own) then run side by side instead of sharing the CUs of XCD 0.
 *                    Results do not depend on it.
 *   readout_norms    a DEVICE scalar holding sum_i ||readout parameter i||_2 as mpqe_step_readout_norms wrote it, or NULL. A
 *                    FORWARD-ONLY step in the chain form with a learned readout and readout_weight_decay > 0 then adds the
 *                    regulariser (model.py:486-490) to loss[0] from it instead of re-forming the four norms in a launch of
 *                    its own per call: a caller that issues many forward-only calls between two parameter updates (the
 *                    reference's loop: eleven margin_loss calls per optimiser step) computes them once. The caller answers
 *                    for the scalar being current. Same arithmetic, same value.
 *   join_event,      join_event != NULL (a hipEvent_t; join_stream a hipStream_t, NULL = the null stream): behind the call's
 *   join_stream      last launch the library records join_event on `stream` and makes join_stream wait for it -- the call ran
 *                    on a side stream, its consumer is enqueued on join_stream. (The other direction -- `stream` waiting for
 *                    the parameters' last writer -- is the caller's.)                                                    */
typedef struct {
    const float *batch_weight[MPQE_STEP_MAX_BATCHES];
    float *query_out;
    uint32_t *notify;
    uint32_t notify_value;
    int32_t xcd_shift;
    void *join_event;
    void *join_stream;
    const float *readout_norms;
} mpqe_step_extra_t;
/* out[0] = sum_i ||p_i||_2 over the learned readout's four parameters (readout_w0, readout_b0, readout_w2, readout_b2 of
 * params_host; reference model.py:486-490), in the order and arithmetic of the step's own regulariser launch. One launch. */
int mpqe_step_readout_norms(const mpqe_step_params_t *params_host, float *out, void *stream);
int mpqe_step_forward_backward_ex(const mpqe_step_params_t *params_host, const mpqe_step_batch_t *batches_host,
                                  int num_batches, const int64_t *anchor_ids, const int64_t *targets,
                                  const int64_t *negs, float margin, const mpqe_step_grads_t *grads_host,
                                  int backward, float *loss, float *scores_pos, float *scores_neg, void *desc,
                                  size_t desc_bytes, int upload_desc, void *workspace, size_t workspace_bytes,
                                  int32_t *err, const mpqe_step_lanes_t *lanes, void *const *events, int num_events,
                                  void *touch, void *stream, const mpqe_step_extra_t *extra_host);

/* The entity-table part of a step's reduction again, from a plan built AFTER the step ran: sums the per-entry gradient
 * rows the step left in `workspace` (its chain launch writes them whatever happens to the plan) per destination row in
 * plan order into grads->tables -- written where the step would have written them (MPQE_STEP_ZERO_GRADS or
 * MPQE_STEP_SPARSE_TABLES in params->flags), added otherwise. For a step that reported MPQE_FLAG_TOUCH_RETRY: same
 * params / batches / desc / workspace as that call (nothing else may have run in the workspace since), `touch` from
 * mpqe_step_touch_build on the same ids. Chain form only. The reference's embedding backward cannot fail
 * (encoders.py:40-43 + autograd); this is what makes the in-step plan equally safe.                            */
int mpqe_step_table_rows(const mpqe_step_params_t *params_host, const mpqe_step_batch_t *batches_host, int num_batches,
                         const mpqe_step_grads_t *grads_host, const void *desc, void *workspace, size_t workspace_bytes,
                         const void *touch, void *stream);

/* margin_loss's regulariser on the readout's parameters (reference model.py:486-490: sum_i ||p_i||_2, unsquared) for the
 * drop-in modules: out[0] += sum_i ||params[i]||_2 (out != NULL; the caller zero-fills it) and / or grads[i] += *grad_out *
 * params[i] / ||params[i]|| (grads != NULL; grad_out: the upstream gradient, one float on the device, NULL = 1). Up to four
 * tensors per call, one workgroup, fixed order of every sum. The fused step computes the same inside its own call.   */
int mpqe_l2_norms(const float *const *params /* host array of device pointers */, const int64_t *sizes /* host */, int count,
                  const float *grad_out, float *out, float *const *grads, void *stream);

/* Ids of the next step from pinned host memory to the device on `stream` (hipMemcpyAsync; stream-ordered, returns at
 * once): the reference moves its index tensors with .to(device) per call (utils.py:17-23). For host mirrors without a
 * HIP binding of their own.                                                                          */
int mpqe_copy_to_device(void *dst, const void *src_host, size_t bytes, void *stream);

/* ---- optimiser step ---------------------------------------------------------
 * reference train.py:83-88: optim.Adam(params, lr) / optim.SGD(params, lr, momentum=0) over every
 * parameter, dense entity tables included. One launch over flat fp32 buffers (the fused step keeps the
 * gradients flat already). Same update rule as torch.optim.Adam (amsgrad off) / torch.optim.SGD:
 *   g += wd p;  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
 * step = t >= 1 (the caller counts). All four arrays [n], updated in place. Hyper-parameters are doubles,
 * as torch holds them: 1 - beta and the bias corrections are formed in double and rounded once.       */
int mpqe_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, double lr,
                   double beta1, double beta2, double eps, double weight_decay, int64_t step, void *stream);
int mpqe_sgd_step(float *param, const float *grad, int64_t n, double lr, double weight_decay, void *stream);
/* Adam over ONLY the entity-table rows a packed step touched ("row-sparse Adam for entity tables"):
 * the distinct (table, row) keys of `touch` (mpqe_step_touch_build). Update rule = torch.optim.SparseAdam's, applied
 * to the per-row gradient sums the step left in grads[t][row]:
 *   m += (1-b1)(g - m);  v += (1-b2)(g g - v);  p -= lr sqrt(1-b2^t)/(1-b1^t) * m / (sqrt(v) + eps)
 * Deviation from the reference's dense Adam (train.py:87), stated: rows that a step does not touch keep their moments
 * undecayed and do not move (dense Adam decays m, v of every row every step and moves rows whose m is non-zero). In
 * exchange a step costs O(touched rows), not 16 bytes x every table element (AM: 191 MB tables, 1M entities: 1 GB).
 * params / grads / exp_avg / exp_avg_sq: [num_modes] host arrays of device pointers, tables [rows_t, dim]; step >= 1. */
int mpqe_adam_rows_step(const void *touch, int64_t num_entries /* of the plan: mpqe_step_touch_entries, or n of
                        mpqe_rows_plan_build */, float *const *params, const float *const *grads, float *const *exp_avg,
                        float *const *exp_avg_sq, int num_modes, int64_t dim, double lr, double beta1, double beta2,
                        double eps, int64_t step, void *stream);

/* ---- the same three updates, refused on the device when the step flagged a fault ------------------------------------
 * reference train_helpers.py:119-120: `loss.backward(); optimizer.step()` (the optimisers of train.py:83-88). The
 * reference's lookups raise IndexError on a bad id BEFORE optimizer.step() is reached; the fused step never raises, it ORs
 * MPQE_FLAG_* into its 4-byte error word, which the host reads when asked -- in the unchecked loop one call late, after
 * the update. These entry points take that word, so a flagged step's gradients (garbage, or table rows missing) never
 * reach the parameters or the moments, with no host synchronisation:
 *   guard    device word, required (NULL: MPQE_ERR_INVALID_ARG). Every workgroup reads it once, before its first
 *            store. Non-zero when the launch executes: the launch writes NOTHING -- param, exp_avg, exp_avg_sq and
 *            *applied keep their bits -- and the call still returns MPQE_OK (the refusal is the device's; the host
 *            learns of it from the word, as before). Zero: exactly the bits the unguarded entry point writes (one
 *            kernel serves both; the unguarded calls pass no word).
 *   applied  optional (NULL: not counted) device counter of the updates that really happened: with a clean word exactly
 *            ONE thread of the launch adds 1 to it, whatever the grid size. An update of several launches passes it to
 *            one of them only.
 * The word must not be written by work that runs CONCURRENTLY with the launch (another stream without an event in
 * between, a peer): workgroups would disagree and the update would be torn. Work earlier on the same stream -- the
 * step itself -- is what it is for. The word is sticky: every guarded update is refused until the host clears it.
 * Everything else (arguments, their checks, the update rules) as in the unguarded calls above.                       */
int mpqe_adam_step_guarded(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, double lr,
                           double beta1, double beta2, double eps, double weight_decay, int64_t step,
                           const int32_t *guard, int64_t *applied, void *stream);
int mpqe_sgd_step_guarded(float *param, const float *grad, int64_t n, double lr, double weight_decay,
                          const int32_t *guard, int64_t *applied, void *stream);
int mpqe_adam_rows_step_guarded(const void *touch, int64_t num_entries, float *const *params, const float *const *grads,
                                float *const *exp_avg, float *const *exp_avg_sq, int num_modes, int64_t dim, double lr,
                                double beta1, double beta2, double eps, int64_t step, const int32_t *guard,
                                int64_t *applied, void *stream);

/* ---- data-parallel exchange of entity-table gradient rows ("exchange touched rows only") ---------
 * Every rank all-gathers the (table, row) keys its packed step touches (key = table << row_bits | row, ~0 = none: the
 * touch plan's sorted keys without repeats, padded) ONCE at pack time and builds one plan over all ranks' keys
 * (mpqe_rows_plan_build: stable sort, so equal keys stay in rank order). Per step each rank all-gathers its gradient
 * rows in its own key order and mpqe_table_rows_sum adds, per key, the gathered rows in plan order into the dense table
 * gradients: the same additions in the same order on every rank -- equal to the dense all-reduce (a sum), bit-identical
 * replicas, and bytes on the wire proportional to the touched rows, not to the tables.                          */
size_t mpqe_rows_plan_bytes(int64_t n);
size_t mpqe_rows_plan_workspace_bytes(int64_t n, int key_bits);
int mpqe_rows_plan_build(const uint64_t *keys /* [n], device */, int64_t n, int row_bits, int key_bits, void *plan,
                         size_t plan_bytes, void *workspace, size_t workspace_bytes, void *stream);
int mpqe_table_rows_sum(const void *plan, int64_t n, const float *rows /* [n, dim] in the order of `keys` */, int64_t dim,
                        float *const *table_grads /* [num_modes] host array of device pointers */, int num_modes,
                        int store /* 1: rows are written, 0: added to */, void *stream);

/* ---- gradient-bucket exchange over peer-mapped buffers (SURVEY.md 5 last row, 8e: "one-hop reduce-scatter + all-gather
 * using all 7 links concurrently ... a custom P2P two-shot over IPC-mapped buffers") ------------------------------------
 * No reference counterpart (the reference is single-process). Every rank of ONE node owns a communication buffer
 * [bucket n floats | world staging slots of one shard | flags] (mpqe_p2p_buffer_bytes; fine-grained device memory from
 * mpqe_p2p_alloc, which also returns its IPC handle) and maps its peers' buffers (mpqe_p2p_open on the handles, exchanged
 * by the host side). mpqe_p2p_allreduce, stream-ordered, per rank: push my contribution to every shard into its owner's
 * slot -> sum the slots of MY shard in rank order and write the sum into that shard of every rank's bucket -> wait until
 * every shard of my bucket has landed. Each byte crosses one link once per direction; the sum of a shard is computed once,
 * so all replicas hold the same bits. epoch: != 0, a new value per call (flags are epoch-stamped, never cleared). phases:
 * 1 push | 2 reduce | 4 wait (7 = the whole exchange; separate phases are for single-process tests). Every poll is
 * bounded: a peer that never arrives ORs MPQE_FLAG_INTERNAL into err (the caller falls back to another collective). */
size_t mpqe_p2p_handle_bytes(void);
size_t mpqe_p2p_buffer_bytes(int64_t n, int world, int64_t *stage_offset, int64_t *flags_offset);
int mpqe_p2p_alloc(size_t bytes, void **ptr, void *handle_out);
int mpqe_p2p_free(void *ptr);
int mpqe_p2p_open(const void *handle, void **mapped);
int mpqe_p2p_close(void *mapped);
int mpqe_p2p_allreduce(void *const *buffers /* [world] host array: buffer of rank p as THIS process addresses it */, int rank,
                       int world, int64_t capacity /* the n the buffers were sized for */, int64_t n /* floats to reduce, <= capacity */,
                       uint32_t epoch, int phases, int32_t *err, void *stream);

/* Glue of the per-step exchange as library launches (the host mirror did it with torch._foreach_copy_ / index_select /
 * where): mpqe_spans_copy: dst[d .. d + n) <- src[s .. s + n) for every span of a DEVICE table of {int64 dst offset, src
 * offset, floats, first workgroup} records (4 096 floats per workgroup; total_blocks = sum of ceil(n / 4096)) -- the
 * touched matrices into the contiguous bucket and back. mpqe_rows_prepare: from the SORTED keys of a touch plan the step
 * built itself, the first key of every run (other slots ~0: fixed size `cap`) and the row of the flat [rows, dim]
 * table-gradient view it names (row_base[table] + row). mpqe_rows_gather: out[i] = rows[gidx[i]].              */
int mpqe_spans_copy(float *dst, const float *src, const void *spans_device, int nspans, int64_t total_blocks, void *stream);
int mpqe_rows_prepare(const uint64_t *sorted_keys, int64_t M, int64_t cap, int row_bits, const int64_t *table_rows /* host */,
                      const int64_t *row_base /* host */, int num_tables, uint64_t *send_keys, int64_t *gidx, void *stream);
int mpqe_rows_gather(const float *rows, const int64_t *gidx, int64_t n, int64_t dim, float *out, void *stream);

/* ---- negative sampling with python's own stream (reference model.py:466-476) -- HOST function, no device work ----------
 * margin_loss draws one negative per query with random.choice(list): CPython's Random.choice is
 * list[_randbelow(len)], _randbelow(n): k = n.bit_length(); r = getrandbits(k); while r >= n: r = getrandbits(k), and
 * getrandbits(k <= 32) is ONE 32-bit Mersenne-Twister output shifted right by 32 - k. The drop-in keeps that stream: the
 * host mirror takes raw outputs from the interpreter's generator (random.getrandbits(32 * n) = n consecutive outputs, the
 * first in the low bits) and this routine replays the rejection loop over them for queries cursor[0] .. nq - 1 in order:
 *   words [nwords] raw outputs; lens_host [nq] list length per query (or NULL: every list has `len_all` entries);
 *   base_host [nq] (or NULL = 0): offset of query i's list in `cand_host`; out_host[i] = cand_host[base + r] (cand_host
 *   NULL: out_host[i] = r, the drawn position).
 * cursor_host[0] (in/out) = next query to serve, cursor_host[1] (out) = words consumed by this call (all of them unless the
 * last query was served first). Returns MPQE_OK, or MPQE_ERR_INVALID_ARG for an empty list (random.choice raises
 * IndexError) or one of 2^32 or more entries. Every pointer is a HOST pointer.                                        */
int mpqe_host_random_choice(const uint32_t *words_host, int64_t nwords, const int64_t *lens_host, int64_t len_all,
                            const int64_t *base_host, const int64_t *cand_host, int64_t nq, int64_t *cursor_host,
                            int64_t *out_host);

/* ---- negative sampling on the device -------------------------------------------
 * reference model.py:466-476: one negative per query, random.choice over query.neg_samples /
 * query.hard_neg_samples (ragged per query) or graph.full_lists[target_mode] (1-chain: one list for all).
 * cand [n_cand]: candidate entity ids. offsets [n_lists + 1] (CSR over cand) or NULL = every query draws
 * from the whole of cand. qidx [nq] (or NULL = identity): list of batch position i. out[i] = a uniform
 * draw from the list, chosen by a counter-based hash of (seed, i) -- stateless, reproduced on the CPU by
 * oracle/ref_cpu.py; NOT python's random stream (same distribution, other numbers). An empty or invalid
 * list ORs MPQE_FLAG_BAD_INDEX into err and writes -1 (the reference raises IndexError).             */
int mpqe_sample_negatives(const int64_t *cand, int64_t n_cand, const int64_t *offsets, int64_t n_lists,
                          const int64_t *qidx, int64_t nq, uint64_t seed, int64_t *out, int32_t *err,
                          void *stream);

/* ---- the GQE baseline: bilinear metapath decoder + set intersection, one launch per formula batch ------------------
 * reference: QueryEncoderDecoder.forward model.py:70-116, BilinearMetapathDecoder decoders.py:123-150, SetIntersection /
 * SimpleSetIntersection decoders.py:270-319, DirectEncoder encoders.py:42-43 (added under ABI 7: entries only).
 * The host compiles a formula into `prog_host`, MPQE_GQE_PROG_INTS int32:
 *   [0] form: 0 = chain (model.py:78-83: the n = B + sum(L) target / negative rows pass through the matrices, row r is
 *       scored against anchor row qrow[r]), 1 = intersection (model.py:84-116: the B queries' anchors pass through the
 *       matrices, query q is scored against row q and rows B + neg_off[q] .. B + neg_off[q + 1] - 1)
 *   [1] branches (1..3)   [2] aggregate over the branches: 0 mean, 1 min   [3] / [4] index of the pre / post matrix of the
 *       intersection (-1: none -- SimpleSetIntersection)   [5] products after the intersection (0..3)
 *   [6] table (mode) of the rows scored against   [8 + 5 b] table of branch b's ids, [9 + 5 b] its products (0..3),
 *       [10 + 5 b ..] their codes; [24 ..] the codes of the products after the intersection.
 *   A code is 2 * matrix index + T: T = 0 multiplies the row by M (decoders.py:145), T = 1 by M^T (project, decoders.py:150).
 *   [7] path operator of every branch site and every site after the intersection: 0 matrix (above), 1 translate
 *       (TransEMetapathDecoder decoders.py:181-208: row + v), 2 scale (BilinearDiagMetapathDecoder decoders.py:211-236:
 *       row * v). With 1 or 2 such a site's code still carries the parameter index in code >> 1 (the low bit is ignored),
 *       mats_host[index] is a [dim] vector (16-byte aligned) and grad_mats_host[index] its [dim] gradient; sites run in
 *       programme order, ((x + v1) + v2) + v3. The pre / post matrices [3] / [4] stay [dim, dim] in the same arrays.
 *   [27] scoring: 0 the cosine, 1 the plain dot product of the two rows (decoders.py:232: no norms, eps not read); -1, which
 *       programmes written before this int existed carry, is the cosine.
 *   Other values of [7] / [27]: MPQE_ERR_INVALID_ARG. Vector gradients: per-workgroup partial column sums over the p_rows
 *   real rows (dY for translate, X * dY for scale), then one ordered pass, site after site in programme order.
 * tables_host / mats_host: host arrays of device pointers ([rows, dim] tables by mode; [dim, dim] matrices), 16-byte
 * aligned. p_ids [branches, p_rows]: the ids that pass through the matrices (chain form: p_rows = n; intersection form:
 * p_rows = B, n >= B); e_ids [e_rows] the other side (chain form: the B anchors; intersection form: e_rows = n). scores [n].
 * dim: a multiple of 16 up to 256, one for every table (MPQE_ERR_UNSUPPORTED otherwise). The cosine and its eps are
 * mpqe_cosine_fwd's; ids are checked as in mpqe_embed_l2norm_fwd (MPQE_FLAG_BAD_NODE_ID, the row becomes zeros), row map
 * entries outside their range OR MPQE_FLAG_BAD_INDEX. save_states != 0 keeps in `workspace` (mpqe_gqe_workspace_bytes,
 * 256-byte aligned) what mpqe_gqe_bwd reads: the input rows of every product, the rows under the aggregate and the
 * scored rows, each [p_rows rounded up to 16, dim]; 0: inference, the workspace is not touched.
 * mpqe_gqe_bwd (same arguments, the workspace of the forward): state gradients in one launch; grad_mats_host[m] +=
 * the products' weight gradients site after site in programme order on mpqe_linear_bwd's fixed-order tiles;
 * grad_tables_host[mode] += per looked-up row the sum of its entries in entry order (one writer per row). No float
 * atomics: the same bits every run. NULL entries are not computed. Arguments are checked before any launch
 * (MPQE_ERR_INVALID_ARG; a short workspace MPQE_ERR_WORKSPACE). */
#define MPQE_GQE_PROG_INTS 32
size_t mpqe_gqe_workspace_bytes(const int32_t *prog_host, int64_t p_rows, int64_t n, int64_t dim);
int mpqe_gqe_fwd(const int32_t *prog_host, const float *const *tables_host, const int64_t *table_rows_host, int num_tables,
                 const int64_t *node_map, int64_t node_map_len, const float *const *mats_host, int num_mats, int64_t dim,
                 const int64_t *p_ids, int64_t p_rows, const int64_t *e_ids, int64_t e_rows, const int64_t *qrow,
                 const int64_t *neg_off, int64_t n, float eps, int save_states, float *scores, void *workspace,
                 size_t workspace_bytes, int32_t *err, void *stream);
int mpqe_gqe_bwd(const int32_t *prog_host, const float *const *tables_host, const int64_t *table_rows_host, int num_tables,
                 const int64_t *node_map, int64_t node_map_len, const float *const *mats_host, int num_mats, int64_t dim,
                 const int64_t *p_ids, int64_t p_rows, const int64_t *e_ids, int64_t e_rows, const int64_t *qrow,
                 const int64_t *neg_off, int64_t n, float eps, const float *grad_scores, float *const *grad_tables_host,
                 float *const *grad_mats_host, void *workspace, size_t workspace_bytes, int32_t *err, void *stream);

/* The rows a programme scores, alone (answering a query: every entity of a mode is a candidate, mpqe_rank_entities does
 * the scoring). The programme's P side exactly as mpqe_gqe_fwd runs it -- lookup, L2 normalisation, the branch products,
 * the intersection, the products after it -- and the rows the forward would score written to out [p_rows, dim] (16-byte
 * aligned; exactly p_rows rows): the forward's arithmetic, instruction for instruction. No E side ([6] of the programme
 * is not read), no workspace, no states. p_ids [branches, p_rows], or NULL with ONE branch: P row r is row r of that
 * branch's table, 0 <= r < p_rows <= its rows, without an id list or node_map -- a whole mode's table projected with no
 * lookups. Bad ids as in the forward (MPQE_FLAG_BAD_NODE_ID, the looked-up row becomes zeros, the other rows are
 * unaffected). Arguments are checked before any launch as in mpqe_gqe_fwd; p_ids == NULL with more than one branch or
 * p_rows above the table's rows: MPQE_ERR_INVALID_ARG (added under ABI 7: an entry only). */
int mpqe_gqe_embed(const int32_t *prog_host, const float *const *tables_host, const int64_t *table_rows_host, int num_tables,
                   const int64_t *node_map, int64_t node_map_len, const float *const *mats_host, int num_mats, int64_t dim,
                   const int64_t *p_ids /* [branches, p_rows], or NULL */, int64_t p_rows, float *out /* [p_rows, dim] */,
                   int32_t *err, void *stream);

/* Queries of DIFFERENT formulas of one query type scored in one launch (added under ABI 7: entries only).
 * mpqe_gqe_fwd_mixed is mpqe_gqe_fwd with save_states == 0 for num_queries queries, query q under programme
 * formula_of[q] (int64 [num_queries] on the device) of num_formulas programmes. The programmes share what the query type
 * fixes -- [0] form, [1] branches, [2] aggregate, [5] and every [9 + 5 b] (the products), [7] operator, [27] scoring, and
 * whether [3] / [4] are present -- and differ in their tables, in the parameter and transposition of every site and in the
 * pre / post matrix. prog_host of the scoring call is any ONE of them (only the shared ints are read).
 * mpqe_gqe_mixed_desc_build checks every programme as mpqe_gqe_fwd does (progs_host [num_formulas, MPQE_GQE_PROG_INTS],
 * tables_host / mats_host as there), refuses programmes that disagree on a shared int with MPQE_ERR_INVALID_ARG before
 * anything is written, and writes one descriptor per formula -- table addresses and rows, the parameter address and
 * transposition of every site -- to `desc` (device memory, 256-byte aligned, mpqe_gqe_mixed_desc_bytes(num_formulas): exact,
 * a byte less is MPQE_ERR_WORKSPACE and nothing is written; 0: num_formulas out of range). The block depends on the
 * programmes and the parameter ADDRESSES only: the caller keeps it between calls, and the host work of a scoring call
 * does not grow with num_formulas. There is no other workspace.
 * Layout of a call: as mpqe_gqe_fwd over the concatenation. Chain form: p_ids [1, n], e_ids [num_queries] the anchors,
 * qrow [n]; intersection form: p_ids [branches, num_queries], e_ids [n], neg_off [num_queries + 1]. The P rows are cut
 * into blocks of 16 and a block into its stretches of one formula; a workgroup owns one stretch (one launch, 16
 * workgroups per block, the spare ones leave at once). scores [n]: every pair's score equals BIT FOR BIT what mpqe_gqe_fwd
 * writes for it when the query's run is handed to it alone with its own programme. A formula index outside
 * [0, num_formulas) -- chain form also a qrow outside [0, num_queries) -- ORs MPQE_FLAG_BAD_INDEX and the pairs of that
 * query score 0; bad ids as in mpqe_gqe_fwd; the other queries' bits are unaffected and nothing is read or written out of
 * bounds. num_queries == 0 (then n == p_rows == e_rows == 0): MPQE_OK, no launch. */
size_t mpqe_gqe_mixed_desc_bytes(int64_t num_formulas);
int mpqe_gqe_mixed_desc_build(const int32_t *progs_host, int64_t num_formulas, const float *const *tables_host,
                              const int64_t *table_rows_host, int num_tables, const float *const *mats_host, int num_mats,
                              int64_t dim, void *desc, size_t desc_bytes, void *stream);
int mpqe_gqe_fwd_mixed(const int32_t *prog_host, int64_t num_formulas, const void *desc, size_t desc_bytes,
                       const int64_t *node_map, int64_t node_map_len, int64_t dim, const int64_t *formula_of,
                       int64_t num_queries, const int64_t *p_ids, int64_t p_rows, const int64_t *e_ids, int64_t e_rows,
                       const int64_t *qrow, const int64_t *neg_off, int64_t n, float eps, float *scores, int32_t *err,
                       void *stream);

/* mpqe_gqe_embed for queries of different formulas (added under ABI 7: an entry only): the rows mpqe_gqe_fwd_mixed would
 * score, written to out [num_queries, dim] (16-byte aligned) in the same single launch and with the same descriptor
 * block, for the intersection form (programme int [0] == 1; the chain form is MPQE_ERR_INVALID_ARG: its candidates are a
 * projected table per formula, which goes by runs through mpqe_gqe_embed). p_ids [branches, num_queries]. Row q equals BIT
 * FOR BIT mpqe_gqe_embed's row when the query's run is handed to it alone with its own programme. A formula index
 * outside [0, num_formulas) ORs MPQE_FLAG_BAD_INDEX and its row is zeros; bad ids as in mpqe_gqe_fwd.
 * num_queries == 0: MPQE_OK, no launch. */
int mpqe_gqe_embed_mixed(const int32_t *prog_host, int64_t num_formulas, const void *desc, size_t desc_bytes,
                         const int64_t *node_map, int64_t node_map_len, int64_t dim, const int64_t *formula_of,
                         int64_t num_queries, const int64_t *p_ids, float *out, int32_t *err, void *stream);

/* Training on GQE queries of DIFFERENT formulas of one query type (csrc/gqe_mixed_train.h; added under ABI 7: entries
 * only): the mixed forward with states and a mixed backward over the layout of mpqe_gqe_fwd_mixed.
 *
 * mpqe_gqe_mixed_index_build writes a second block beside the descriptor block: per formula the table INDEX of the four
 * slots and the parameter INDEX of every site (`index`: device memory, 256-byte aligned, mpqe_gqe_mixed_index_bytes:
 * exact, a byte less is MPQE_ERR_WORKSPACE and nothing is written; programmes that disagree on a shared int are refused
 * before anything is written). It depends on the programmes only: the caller keeps it for the life of the formula list.
 *
 * mpqe_gqe_fwd_mixed_save is mpqe_gqe_fwd_mixed (every score the same BITS) and keeps in `workspace` (256-byte aligned,
 * mpqe_gqe_mixed_train_workspace_bytes: exact, 0 for arguments out of range) what mpqe_gqe_fwd(save_states = 1) keeps,
 * indexed by P row of the concatenation; a stretch writes its own rows only. num_tables / num_mats: the lengths of the
 * lists the blocks were built on (they size the workspace).
 *
 * mpqe_gqe_bwd_mixed (the forward's operands and workspace): grad_tables_host [num_tables] / grad_mats_host [num_mats]
 * are host arrays of device pointers, NULL = neither computed nor written; gradients are ADDED. State gradients in one
 * launch: every dY and GE row is bit for bit what mpqe_gqe_bwd computes when the query's run is handed to it alone (a
 * row's arithmetic depends neither on its tile row nor on its tile's other rows). Parameter gradients: the contributions
 * (site in site order, P row) of the queries with a valid formula index are sorted stably by parameter index and summed
 * in chunks of MPQE_GQE_MIX_GRAD_CHUNK consecutive contributions in list order (v_mfma_f32_16x16x4_f32), the chunk sums
 * in chunk order, then added to the buffer; table rows: per (table index << 40 | row) the entries (branch sources in
 * branch order, then the E row of every pair) in entry order, one writer per row. No float atomics: the order of every
 * addition is a function of (formula_of, programmes) alone, the bits are the same every run and do not depend on what
 * the workspace held. A formula index outside [0, num_formulas) -- chain form also a qrow outside [0, num_queries) --
 * ORs MPQE_FLAG_BAD_INDEX and the query contributes no gradient anywhere; a bad id's row is zeros and gets no table
 * gradient. num_queries == 0: MPQE_OK, no launch. Arguments are checked before any launch; a short workspace or block is
 * MPQE_ERR_WORKSPACE and nothing is written. */
#define MPQE_GQE_MIX_GRAD_CHUNK 64
size_t mpqe_gqe_mixed_index_bytes(int64_t num_formulas);
int mpqe_gqe_mixed_index_build(const int32_t *progs_host, int64_t num_formulas, int num_tables, int num_mats, int64_t dim,
                               void *index, size_t index_bytes, void *stream);
size_t mpqe_gqe_mixed_train_workspace_bytes(const int32_t *prog_host, int64_t num_formulas, int num_tables, int num_mats,
                                            int64_t p_rows, int64_t n, int64_t dim);
int mpqe_gqe_fwd_mixed_save(const int32_t *prog_host, int64_t num_formulas, const void *desc, size_t desc_bytes,
                            int num_tables, int num_mats, const int64_t *node_map, int64_t node_map_len, int64_t dim,
                            const int64_t *formula_of, int64_t num_queries, const int64_t *p_ids, int64_t p_rows,
                            const int64_t *e_ids, int64_t e_rows, const int64_t *qrow, const int64_t *neg_off, int64_t n,
                            float eps, float *scores, void *workspace, size_t workspace_bytes, int32_t *err, void *stream);
int mpqe_gqe_bwd_mixed(const int32_t *prog_host, int64_t num_formulas, const void *desc, size_t desc_bytes,
                       const void *index, size_t index_bytes, int num_tables, int num_mats, const int64_t *node_map,
                       int64_t node_map_len, int64_t dim, const int64_t *formula_of, int64_t num_queries,
                       const int64_t *p_ids, int64_t p_rows, const int64_t *e_ids, int64_t e_rows, const int64_t *qrow,
                       const int64_t *neg_off, int64_t n, float eps, const float *grad_scores,
                       float *const *grad_tables_host, float *const *grad_mats_host, void *workspace,
                       size_t workspace_bytes, int32_t *err, void *stream);

/* R-GCN queries of DIFFERENT formulas of one query type scored in two launches, forward only (csrc/rgcn_mixed.hip; added
 * under ABI 7: entries only). The formulas of a query type share the template, the pass count, the layers and the readout;
 * a formula's own part is one record of MPQE_RGCN_MIX_REC_INTS int32:
 *   [0..2] the relation id of every template edge (mpqe_template_info's edge order, as edge_type_host of
 *          mpqe_rgcn_template_fwd), [3..5] the table index of every anchor slot, [6..8] the mode-embedding row of every
 *          variable slot, [9] the target mode's table index. Entries past the template's edges / anchors / variables
 *          are not read.
 * mpqe_rgcn_mixed_desc_build range-checks every field read (relation >= 0, table index in [0, num_tables), row in
 * [0, mode_emb_rows); tables non-NULL with table_rows >= 0: MPQE_ERR_INVALID_ARG; a table that is not 16-byte aligned:
 * MPQE_ERR_UNSUPPORTED) before anything is written, and writes one descriptor per formula to `desc` (device memory,
 * 256-byte aligned, mpqe_rgcn_mixed_desc_bytes(num_formulas): exact, a byte less is MPQE_ERR_WORKSPACE and nothing is
 * written; 0: num_formulas out of range). The block holds ADDRESSES and indices only: the caller keeps it between calls
 * and rebuilds it when a table has moved; a scoring call does no host work per formula.
 *
 * Operands of a scoring call: node_map / node_map_len as in mpqe_embed_l2norm_fwd; mode_emb the mode embeddings (at least
 * the mode_emb_rows of the build); basis_host / root_host / bias_host HOST arrays of `passes` device pointers -- entry p
 * is the layer pass p runs (basis [num_relations, dim, dim], root [dim, dim], bias [dim] or NULL; bias_host itself may be
 * NULL); ReLU after every pass but the last; readout MPQE_READOUT_TM / _SUM / _MAX; formula_of [num_queries] int64 and
 * anchors [num_queries, A] int64 on the device. The queries are cut into blocks of 64 and a block into its stretches of
 * one formula; a workgroup owns one stretch and runs its whole programme (64 workgroups per block, the spare ones leave at
 * once; no pre-pass). workspace: mpqe_rgcn_mixed_workspace_bytes(query_type, num_queries, dim) -- exact: two node-state
 * buffers and the query embeddings; 0: arguments out of range --, 16-byte aligned. mpqe_rgcn_embed_mixed runs the encode
 * launch alone and writes the query embeddings to q_out [num_queries, dim]; mpqe_rgcn_fwd_mixed runs both launches:
 * ids [n] / qrow [n] in the layout of forward() (row i is the pair of query qrow[i] and entity ids[i] of that query's
 * target mode), scores [n].
 *   bits       every score (every q_out element) equals BIT FOR BIT what the module path writes for it when the query's
 *              run is handed to it alone: mpqe_embed_l2norm_fwd + mpqe_var_rows_fwd -> mpqe_rgcn_template_fwd per pass ->
 *              mpqe_readout_fwd -> mpqe_embed_l2norm_fwd + mpqe_cosine_fwd.
 *   shapes     dim % 4 == 0, mode_emb, every matrix and the workspace 16-byte aligned, 1 <= passes <= 4, readout one of
 *              the three, num_queries < 2^25, n < 2^32: MPQE_ERR_UNSUPPORTED otherwise, before any launch.
 *   bad index  a formula_of[q] outside [0, num_formulas) or a qrow[i] outside [0, num_queries) ORs MPQE_FLAG_BAD_INDEX
 *              and the pairs concerned score 0 (the query's q_out row is zeros). A descriptor's relation outside
 *              [0, num_relations) ORs MPQE_FLAG_BAD_RELATION with the same result.
 *   bad ids    MPQE_FLAG_BAD_NODE_ID, the looked-up row becomes zeros, as on the module path.
 *   The other queries' bits are unaffected and nothing is read or written out of bounds. num_queries == 0 (then n == 0):
 *   MPQE_OK, no launch. Arguments are checked before any launch; a short descriptor block or workspace:
 *   MPQE_ERR_WORKSPACE. The result does not depend on what the workspace held. */
#define MPQE_RGCN_MIX_REC_INTS 10
size_t mpqe_rgcn_mixed_desc_bytes(int64_t num_formulas);
int mpqe_rgcn_mixed_desc_build(int query_type, const int32_t *recs_host, int64_t num_formulas,
                               const float *const *tables_host, const int64_t *table_rows_host, int num_tables,
                               int64_t mode_emb_rows, void *desc, size_t desc_bytes, void *stream);
size_t mpqe_rgcn_mixed_workspace_bytes(int query_type, int64_t num_queries, int64_t dim);
int mpqe_rgcn_embed_mixed(int query_type, int64_t num_formulas, const void *desc, size_t desc_bytes,
                          const int64_t *node_map, int64_t node_map_len, const float *mode_emb,
                          const float *const *basis_host, const float *const *root_host, const float *const *bias_host,
                          int64_t num_relations, int passes, int readout, int64_t dim, const int64_t *formula_of,
                          const int64_t *anchors, int64_t num_queries, void *workspace, size_t workspace_bytes,
                          float *q_out /* [num_queries, dim] */, int32_t *err, void *stream);
int mpqe_rgcn_fwd_mixed(int query_type, int64_t num_formulas, const void *desc, size_t desc_bytes, const int64_t *node_map,
                        int64_t node_map_len, const float *mode_emb, const float *const *basis_host,
                        const float *const *root_host, const float *const *bias_host, int64_t num_relations, int passes,
                        int readout, int64_t dim, const int64_t *formula_of, const int64_t *anchors, int64_t num_queries,
                        const int64_t *ids, const int64_t *qrow, int64_t n, float eps, void *workspace,
                        size_t workspace_bytes, float *scores, int32_t *err, void *stream);

/* Training on R-GCN queries of DIFFERENT formulas of one query type (csrc/rgcn_mixed_train.h; added under ABI 7: entries
 * only): the mixed forward with states and a mixed backward. Operands as in mpqe_rgcn_fwd_mixed unless said otherwise.
 *
 * mpqe_rgcn_mixed_index_build writes a second block beside the descriptor block from the same records: per formula the
 * table INDEX of every anchor slot and of the target mode, the relation of every edge and the mode-embedding row of every
 * variable slot (`index`: device memory, 256-byte aligned, mpqe_rgcn_mixed_index_bytes: exact, 0 for num_formulas out of
 * range, a byte less is MPQE_ERR_WORKSPACE and nothing is written; a negative field read: MPQE_ERR_INVALID_ARG). It
 * depends on the records only: the caller keeps it for the life of the formula list.
 *
 * Sizes of a training call: num_tables (the table list the descriptor block was built on), mode_emb_rows, num_layers
 * (distinct parameter sets, 1 .. 4) and n, the pairs: ids [n] = num_queries targets, then the negatives in CSR order under
 * neg_off [num_queries + 1], n = num_queries + neg_off[num_queries] (forward()'s layout), or n = 0: nothing is scored.
 * workspace: 256-byte aligned, mpqe_rgcn_mixed_train_workspace_bytes -- exact; 0: arguments out of range.
 *
 * mpqe_rgcn_fwd_mixed_save is mpqe_rgcn_fwd_mixed with the pair layout fixed so (it takes neg_off, not qrow): every score
 * is the same BITS mpqe_rgcn_fwd_mixed writes for the equivalent qrow. It keeps in the workspace every pass's node states
 * (passes + 1 buffers [num_queries * N, dim]) and the query embeddings; q_out, when not NULL, receives a copy of those
 * [num_queries, dim]. Under the target-message readout the last pass still computes the target slot alone; the backward
 * never reads the slots nobody wrote. A negative whose offsets do not name a query ORs MPQE_FLAG_BAD_INDEX and scores 0.
 *
 * mpqe_rgcn_bwd_mixed takes the forward's operands and workspace, plus layer_of_pass_host [passes] (which of the
 * num_layers parameter sets a pass ran, each in [0, num_layers)), grad_scores [n] OR grad_q [num_queries, dim] -- exactly
 * one non-NULL; with grad_q the score phase is skipped and ids / neg_off are not read -- and the gradient buffers:
 * grad_tables_host [num_tables], grad_mode_emb [mode_emb_rows, dim], grad_basis_host / grad_root_host / grad_bias_host
 * [num_layers] (host arrays of device pointers; the arrays themselves may be NULL). NULL = neither computed nor written;
 * gradients are ADDED. Every buffer 16-byte aligned.
 *   states     one launch, a workgroup per stretch of one formula, found as the forward finds it: the cosine backward of
 *              the stretch's pairs, one wave per pair, a query's terms summed in the order target, then its negatives in
 *              CSR order; the readout backward (max: the lowest node on ties, from the saved last state); per pass from the
 *              last the ReLU mask from the saved state and the layer's transposed product, on the stretch alone.
 *   parameters the contributions (pass, slot, query) -- the slots the template's edges in edge order, then the node slots
 *              for the root term; x_p[query, src] (x) g_{p+1}[query, dst] -- carry the key layer_of_pass[p] *
 *              (num_relations + 1) + relation (num_relations: the root); sorted stably by key, cut into chunks of
 *              MPQE_RGCN_MIX_GRAD_CHUNK consecutive contributions, a chunk summed in list order from a zero accumulator
 *              (v_mfma_f32_16x16x4_f32), the chunk sums added in chunk order, the total added to the buffer by the one
 *              workgroup that owns the strip. bias: the column sums of the g rows of the layer's root contributions, mode
 *              embeddings: of the variable slots' (slot, query) rows per row, both in the same chunked order.
 *   table rows per (table index << 40 | row) the entries -- the anchors in (slot, query) order, then the pairs in pair
 *              order -- summed in entry order through the l2-norm backward, one writer per row.
 *   No float atomics: the order of every addition is a function of (formula_of, records, neg_off) alone, the bits are the
 *   same every run and do not depend on what the workspace held beyond what the save call wrote.
 *   bad input  a formula index outside [0, num_formulas) ORs MPQE_FLAG_BAD_INDEX, a descriptor's relation outside
 *              [0, num_relations) MPQE_FLAG_BAD_RELATION (a stretch whose neg_off entries do not ascend inside
 *              [0, n - num_queries]: MPQE_FLAG_BAD_INDEX): the query contributes NO gradient anywhere. A bad id's row is
 *              zeros and gets no table gradient. The other queries' bits are unaffected.
 *   shapes     dim a multiple of 16 in [16, 256], 1 <= passes <= 4, the three readouts, num_layers <= 4, n < 2^31:
 *              MPQE_ERR_UNSUPPORTED otherwise, before any launch. num_queries == 0 (then n == 0): MPQE_OK, no launch.
 *   Arguments are checked before any launch; a short block or workspace is MPQE_ERR_WORKSPACE and nothing is written. */
#define MPQE_RGCN_MIX_GRAD_CHUNK 64
size_t mpqe_rgcn_mixed_index_bytes(int64_t num_formulas);
int mpqe_rgcn_mixed_index_build(int query_type, const int32_t *recs_host, int64_t num_formulas, void *index,
                                size_t index_bytes, void *stream);
size_t mpqe_rgcn_mixed_train_workspace_bytes(int query_type, int64_t num_queries, int64_t n, int64_t dim, int passes,
                                             int64_t num_relations, int num_tables, int64_t mode_emb_rows, int num_layers);
int mpqe_rgcn_fwd_mixed_save(int query_type, int64_t num_formulas, const void *desc, size_t desc_bytes,
                             const int64_t *node_map, int64_t node_map_len, const float *mode_emb,
                             const float *const *basis_host, const float *const *root_host, const float *const *bias_host,
                             int64_t num_relations, int passes, int readout, int64_t dim, const int64_t *formula_of,
                             const int64_t *anchors, int64_t num_queries, const int64_t *ids, const int64_t *neg_off,
                             int64_t n, float eps, int num_tables, int64_t mode_emb_rows, int num_layers, void *workspace,
                             size_t workspace_bytes, float *scores, float *q_out, int32_t *err, void *stream);
int mpqe_rgcn_bwd_mixed(int query_type, int64_t num_formulas, const void *desc, size_t desc_bytes, const void *index,
                        size_t index_bytes, const int64_t *node_map, int64_t node_map_len, const float *mode_emb,
                        const float *const *basis_host, const float *const *root_host, const float *const *bias_host,
                        int64_t num_relations, int passes, int readout, int64_t dim, const int64_t *formula_of,
                        const int64_t *anchors, int64_t num_queries, const int64_t *ids, const int64_t *neg_off, int64_t n,
                        float eps, int num_tables, int64_t mode_emb_rows, int num_layers, const int *layer_of_pass_host,
                        const float *grad_scores, const float *grad_q, float *const *grad_tables_host,
                        float *grad_mode_emb, float *const *grad_basis_host, float *const *grad_root_host,
                        float *const *grad_bias_host, void *workspace, size_t workspace_bytes, int32_t *err, void *stream);

/* ---- exact answers of a conjunctive query on the knowledge graph (csrc/kg.hip) ------------------------------------
 * reference: Graph.get_metapath_neighs graph.py:459-473 (the answer set of a chain) and Graph.get_negative_samples
 * graph.py:263-314 (intersection / union of the branch sets; negatives = full set - answers, hard negatives = union -
 * intersection). Integer work only; added under ABI 7: entries only.
 * Row space: everything is in TABLE ROWS of a mode (node_maps[id]), as in mpqe_rank_entities. A set of entities of a mode
 * with n rows is a bitmap of W = ceil(n / 32) uint32 words, row r = bit r % 32 of word r / 32; bits at or above n are
 * always written as 0. mode_rows_host [num_modes <= 16]: n per mode, 1 .. 2^30.
 * Adjacency: one CSR per typed relation (m1, name, m2): rel_offsets_host[i] -> int64 [rows(m1) + 1] and rel_rows_host[i]
 * -> int64 [rel_edges_host[i]] on the device (the three arrays themselves on the host); values are rows of m2, in any
 * order, repeats allowed. A row without neighbours has an empty list and contributes nothing (graph.py:467).
 * Programme: the MPQE_GQE_PROG_INTS int32 layout of mpqe_gqe_fwd -- [1] branches (1..3), [5] hops after the merge (0..1),
 * [6] target mode, [8 + 5 b] mode of branch b's anchor, [9 + 5 b] its hops (1..3), [10 + 5 b ..] their codes, [24] the
 * code of the hop after the merge -- with code = relation index << 4 | destination mode where GQE has a matrix code.
 * Hops walk from the anchors to the target: for a query edge (x, rel, y) the hop uses the CSR of reverse_relation(rel).
 * The branches must end in one mode and the last hop in the target mode (MPQE_ERR_INVALID_ARG otherwise).
 *   anchor_rows [branches, Q] int64 (device): the anchors' rows. A row outside its mode ORs MPQE_FLAG_BAD_INDEX into err
 *               and gives THAT query empty sets; the other queries are unaffected. A CSR offset or row outside
 *               its range is flagged too and not followed.
 *   answers [Q, W(target mode)]: the query's exact answer set.
 *   hard    [Q, W] or NULL: the same programme with the merge taken as OR, minus answers (union_neighs - inter_neighs;
 *               3-chain_inter: union_pos_nodes - pos_nodes, graph.py:299-311); all zero with one branch.
 *   counts  [2, Q] int64 or NULL: population counts of answers, then of hard (0 when hard is NULL).
 *   flags   MPQE_KG_GLOBAL_BITS: keep the working bitmaps in the workspace, not in LDS (the form modes above 77 824 rows
 *               take anyway; for tests at small shapes).
 *   workspace: what the size query returns for the same flags (256 when the bitmaps live in LDS: not touched); NOT
 *               assumed zeroed. Every word of every output is written; the result is a set -- the same bits every run.
 * num_queries == 0: nothing is launched. Arguments are checked before any launch (MPQE_ERR_INVALID_ARG; a short
 * workspace MPQE_ERR_WORKSPACE; the size query returns 0). */
#define MPQE_KG_GLOBAL_BITS 1
size_t mpqe_kg_workspace_bytes(const int32_t *prog_host, int64_t num_queries, const int64_t *mode_rows_host, int num_modes,
                               int flags);
int mpqe_kg_answers(const int32_t *prog_host, const int64_t *const *rel_offsets_host, const int64_t *const *rel_rows_host,
                    const int64_t *rel_edges_host, int num_rels, const int64_t *mode_rows_host, int num_modes,
                    const int64_t *anchor_rows /*[branches, Q] device*/, int64_t num_queries, uint32_t *answers /*[Q, W]*/,
                    uint32_t *hard /*[Q, W] or NULL*/, int64_t *counts /*[2, Q] or NULL*/, int flags, void *workspace,
                    size_t workspace_bytes, int32_t *err, void *stream);

/* Bitmaps [Q, W] of a mode with n rows -> the CSR mpqe_rank_entities takes as excl_offsets / excl_rows: query q's rows
 * ascending at rows_out[offsets[q] .. offsets[q + 1]). `select`, with valid [W] (NULL: every row below n) marking the rows
 * that are entities:   MPQE_KG_ROWS_SET         the set itself
 *                      MPQE_KG_ROWS_COMPLEMENT  valid & ~bits: the plain negatives (full_sets[mode] - answers); table
 *                                               holes never become negatives
 *                      MPQE_KG_ROWS_WITH_HOLES  bits | ~valid: the set and every row below n that is no entity (what a
 *                                               filtered ranking excludes)
 * offsets [Q + 1] is the caller's exclusive scan of the lists' lengths (mpqe_kg_answers' counts); rows_cap the slots
 * behind rows_out. A list that does not fit its segment, or a segment outside [0, rows_cap], ORs MPQE_FLAG_BAD_INDEX
 * into err and nothing is written outside the segment. */
#define MPQE_KG_ROWS_SET 0
#define MPQE_KG_ROWS_COMPLEMENT 1
#define MPQE_KG_ROWS_WITH_HOLES 2
int mpqe_kg_rows(const uint32_t *bits, int64_t num_queries, int64_t n, const uint32_t *valid /*[W] or NULL*/, int select,
                 const int64_t *offsets /*[Q + 1]*/, int64_t *rows_out, int64_t rows_cap, int32_t *err, void *stream);

/* ---- sampling on the KG index (csrc/kg_sample.hip) -- added under ABI 7: entries only --------------------------------
 * Conventions of mpqe_kg_answers: every set, id and offset is in table ROWS; the *_host arrays are host arrays (of device
 * pointers); a CSR offset or row outside its range ORs MPQE_FLAG_BAD_INDEX and is not followed; arguments are checked
 * before any launch. Integer work only.
 *
 * The random stream. M = the splitmix64 finaliser of mpqe_sample_negatives (x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) *
 * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) * 0x94D049BB133111EB; x ^ x >> 31; all mod 2^64). With base = M[seed ^ M[slot]]:
 *   the walk          draw number d = 0, 1, ... of try t of a slot is  M[ M[base ^ t] ^ d ] % length
 *   the row sampler   round r = 0 .. 7 of query q's Feistel network uses  M[ base ^ ((r + 1) << 32 | R) ] & (2^h - 1)
 * Stateless: an output is a pure function of (seed, slot, the graph or set). tests/kg_sample_oracle.py restates both.
 *
 * mpqe_kg_sample_queries: grounded queries by the reference's random walk (Graph.sample_query_subgraph_bytype
 * graph.py:321-389). The CSR arrays are mpqe_kg_answers'; rel_src_mode_host / rel_dst_mode_host [num_rels] the modes of
 * every typed relation; rel_start_rows_host[i] -> int64 [rel_start_count_host[i]] on the device: relation i's source rows
 * with a non-empty list, ascending. num_rels <= 4 096, num_modes <= 16, 1 <= max_tries <= 1 024.
 * out [num_slots, MPQE_KG_QUERY_INTS] int64: [0] 1 = a query, 0 = none after max_tries; then the query's edges (source row,
 * relation index, destination row) in the order of the reference's query tuple with nested tuples flattened (3-inter_chain:
 * edge_1, edge_2, the edge from edge_2's neighbour; 3-chain_inter: the first edge, the two intersection edges). Unused
 * ints, and everything behind a status of 0, are -1. The target is edge 0's source row.
 * One try (draws in this order, each uniform by the stream above):
 *   start   a relation among those with rel_start_count > 0 (in index order; a relation without edges is skipped, where
 *           the reference's random.choice([]) would raise), then one of its start rows.
 *   flat    the "flat adjacency" of row x of mode m is the concatenation, in relation-index order, of x's lists in every
 *           relation whose source mode is m; a draw from it is uniform over its ENTRIES (graph.py:147-151).
 *   edges   1-chain: 1 entry at the start; 2-chain / 3-chain: 1 at the start, then 1 at each neighbour in turn; 2-inter /
 *           3-inter: 2 / 3 at the start; 3-inter_chain: 2 at the start, then 1 at the second's neighbour; 3-chain_inter:
 *           1 at the start, 2 at its neighbour. Fewer entries than needed at a node rejects the try. The edges out of one
 *           node are redrawn until their (relation, neighbour) pairs differ; since the index allows repeated entries an
 *           edge gives up after 64 redraws and the try is rejected (a walk never spins).
 * A corrupt offset / row rejects that try only. workspace: mpqe_kg_sample_workspace_bytes (0: arguments out of range),
 * 8-byte aligned; the host writes the per-relation table into it on `stream` with every call. */
#define MPQE_KG_QUERY_INTS 10
size_t mpqe_kg_sample_workspace_bytes(int num_rels, int num_modes);
int mpqe_kg_sample_queries(const int64_t *const *rel_offsets_host, const int64_t *const *rel_rows_host,
                           const int64_t *rel_edges_host, const int32_t *rel_src_mode_host, const int32_t *rel_dst_mode_host,
                           const int64_t *const *rel_start_rows_host, const int64_t *rel_start_count_host, int num_rels,
                           const int64_t *mode_rows_host, int num_modes, int query_type, int64_t num_slots, int max_tries,
                           uint64_t seed, int64_t *out /*[num_slots, 10] device*/, void *workspace, size_t workspace_bytes,
                           int32_t *err, void *stream);

/* mpqe_kg_rows with a bound: at most k members of every query's selected set (the reference's Query(neg_sample_max):
 * random.sample of the negatives, graph.py:83-87). select: MPQE_KG_ROWS_SET or MPQE_KG_ROWS_COMPLEMENT
 * (MPQE_KG_ROWS_WITH_HOLES: MPQE_ERR_INVALID_ARG). For query q with c selected members, m = min(k, c) rows are written to
 * rows_out[offsets[q] .. offsets[q] + m); offsets[q + 1] - offsets[q] must be m (otherwise MPQE_FLAG_BAD_INDEX, and
 * nothing is written outside the segment). c <= k: all members ascending, the bits of mpqe_kg_rows. c > k: k DISTINCT
 * members, a uniform k-subset in the order j = 0 .. k - 1 of their draw: the member of rank P[j] for the bijection P of
 * [0, c) keyed by (seed, q): with h the least integer >= 1 with 4^h >= c, x = j is split into L = x >> h, R = x & (2^h - 1),
 * eight rounds (L, R) <- (R, L ^ F_r[R]) with F_r from the stream above, x = L << h | R, repeated while x >= c.
 * 1 <= k <= MPQE_KG_SAMPLE_MAX_K, n <= MPQE_KG_SAMPLE_MAX_ROWS: MPQE_ERR_UNSUPPORTED above either; k < 1:
 * MPQE_ERR_INVALID_ARG. */
#define MPQE_KG_SAMPLE_MAX_K 1024
#define MPQE_KG_SAMPLE_MAX_ROWS (1 << 22)
int mpqe_kg_sample_rows(const uint32_t *bits, int64_t num_queries, int64_t n, const uint32_t *valid /*[W] or NULL*/,
                        int select, const int64_t *offsets /*[Q + 1]*/, int64_t *rows_out, int64_t rows_cap, int k,
                        uint64_t seed, int32_t *err, void *stream);

/* ---- queries of DIFFERENT formulas in one launch (csrc/kg.hip, csrc/kg_sample.hip) -- added under ABI 7: entries only -----
 * mpqe_kg_answers and mpqe_kg_sample_rows take one formula (one mode) a launch; a sampled batch on a schema of ~100 typed
 * relations meets nearly as many formulas as it has queries. These entries fix only the QUERY TYPE per launch and take the
 * relations from every query's own record, through a device table of the index built once.
 *
 * mpqe_kg_table_build: the table (mpqe_kg_table_bytes; 0: num_rels outside 1 .. 4 096 or num_modes outside 1 .. 16; 8-byte
 * aligned). Per relation: the CSR pointers and edge count of mpqe_kg_answers, the row counts and indices of its two modes,
 * and rel_reverse_host[i], the index of reverse_relation(relation i) in the same index (-1: absent). Per mode: its row count,
 * mode_valid_host[m] -> uint32 [W(m)] on the device, the rows that are entities (the array or an entry NULL: all), and
 * mode_row_ids_host[m] -> int64 [n] row -> entity id (NULL: none; ids_out below then holds -1). The host writes the table
 * on `stream`; it is read-only afterwards and holds device addresses, so it lives as long as the arrays it names.
 *
 * mpqe_kg_answers_mixed: one workgroup per query. records [Q, MPQE_KG_QUERY_INTS] int64 (device) in exactly the layout
 * mpqe_kg_sample_queries writes; read are the status, the relation indices, the destination rows of the leaf edges (the
 * anchors) and edge 0's source row (the probe). The hop structure is query_type's, hops in the order of kg.query_hops: the hop
 * for query edge (x, rel, y) walks the CSR of table[rel].reverse.
 *   1-chain e0 | 2-chain e1, e0 | 3-chain e2, e1, e0 | 2-inter e0 & e1 | 3-inter e0 & e1 & e2 | 3-inter_chain e0 & (e2, e1) |
 *   3-chain_inter (e1 & e2), then e0
 *   status 0       empty sets, counts 0, target_mode -1, member 0; no flag.
 *   malformed      a status other than 0 / 1, a relation index outside the table, a missing reverse, a relation whose source
 *                  mode is not the frontier's, branches that end in different modes, an anchor outside its mode, a CSR
 *                  offset or row outside its range: MPQE_FLAG_BAD_INDEX is ORed into err, THAT query gets what status 0
 *                  gets, the other queries are unaffected.
 *   answers, hard  [Q, out_words] or NULL, out_words >= W(widest mode of the index). Every word is written; the words at or
 *                  above the query's own W(target mode) are 0. With both NULL no bitmap leaves the workgroup.
 *   counts         [2, Q] int64 or NULL: |answers|, |hard|; |hard| is 0 unless `hard` is given or flags has
 *                  MPQE_KG_COUNT_HARD (the hard flavour is then walked for its count alone).
 *   target_mode    [Q] int32: the mode the query's walk ends in, -1 for a query that produced nothing.
 *   member         [Q] int32 or NULL: 1 if probe_rows[q] (probe_rows NULL: the record's target row, edge 0's source) is in
 *                  the answer set; a probe outside the mode gives 0.
 *   flags          MPQE_KG_GLOBAL_BITS as for mpqe_kg_answers (LDS holds the working bitmaps up to 2 432 words of the
 *                  WIDEST mode), MPQE_KG_COUNT_HARD.
 *   workspace      mpqe_kg_mixed_workspace_bytes for the same flags (0: arguments out of range; 256 when the bitmaps live in
 *                  LDS: not touched); not assumed zeroed. No spin waits, no float work; the same bits every run.
 * num_queries == 0: nothing is launched. mode_rows_host must be the array the table was built from (the kernel refuses a
 * relation whose bitmaps would not fit: malformed).
 *
 * mpqe_kg_sample_rows_mixed: mpqe_kg_sample_rows with n and valid taken per query from mode_of_query [Q] int32 and the table,
 * query q's bitmap at bits + q * bits_stride words (bits_stride >= W(widest mode)), and q_base (>= 0) added to the query's
 * position in the draw key: the bijection is keyed by (seed, q_base + q), so a batch cut into chunks draws what the whole
 * batch draws. The draw itself is unchanged. A query of mode -1 must have an empty segment (MPQE_FLAG_BAD_INDEX otherwise);
 * a mode outside [-1, num_modes) is flagged and nothing is written. rows_out and ids_out may each be NULL; ids_out receives
 * the same lists as entity ids through the table's row -> id arrays. */
#define MPQE_KG_COUNT_HARD 2
size_t mpqe_kg_table_bytes(int num_rels, int num_modes);
int mpqe_kg_table_build(const int64_t *const *rel_offsets_host, const int64_t *const *rel_rows_host,
                        const int64_t *rel_edges_host, const int32_t *rel_src_mode_host, const int32_t *rel_dst_mode_host,
                        const int32_t *rel_reverse_host, int num_rels, const int64_t *mode_rows_host,
                        const uint32_t *const *mode_valid_host, const int64_t *const *mode_row_ids_host, int num_modes,
                        void *table, size_t table_bytes, void *stream);
size_t mpqe_kg_mixed_workspace_bytes(int64_t num_queries, const int64_t *mode_rows_host, int num_modes, int flags);
int mpqe_kg_answers_mixed(const void *table, const int64_t *mode_rows_host, int num_modes, int query_type,
                          const int64_t *records /*[Q, 10] device*/, int64_t num_queries,
                          const int64_t *probe_rows /*[Q] or NULL*/, uint32_t *answers /*[Q, out_words] or NULL*/,
                          uint32_t *hard /*[Q, out_words] or NULL*/, int64_t out_words, int64_t *counts /*[2, Q] or NULL*/,
                          int32_t *target_mode /*[Q]*/, int32_t *member /*[Q] or NULL*/, int flags, void *workspace,
                          size_t workspace_bytes, int32_t *err, void *stream);
int mpqe_kg_sample_rows_mixed(const void *table, const int64_t *mode_rows_host, int num_modes, const uint32_t *bits,
                              int64_t bits_stride, const int32_t *mode_of_query /*[Q]*/, int64_t num_queries, int64_t q_base,
                              int select, const int64_t *offsets /*[Q + 1]*/, int64_t *rows_out, int64_t *ids_out,
                              int64_t rows_cap, int k, uint64_t seed, int32_t *err, void *stream);

/* ---- the neighbourhood-aggregating entity encoder on the KG index (csrc/sage.hip) -- added under ABI 7: entries only ------
 * reference: utils.get_encoder utils.py:97-130, Encoder encoders.py:47-129, MeanAggregator aggregators.py:17-68 (`--depth
 * 1..3`). Conventions of the KG and GQE entries above: *_host arrays are host arrays (of device pointers); everything is in
 * table ROWS; arguments are checked before any launch (MPQE_ERR_INVALID_ARG / MPQE_ERR_UNSUPPORTED / MPQE_ERR_WORKSPACE; the
 * size query returns 0); a bad offset or row ORs MPQE_FLAG_BAD_INDEX into err and is not followed; every word of every output
 * is written; the workspace is not assumed zeroed; no float atomics: a call gives the same bits every run.
 *
 * mpqe_kg_sample_neighbours: the draws of MeanAggregator.forward (aggregators.py:51-53) for the R relations
 * use_rels_host[0 .. R) (indices into the index's relations, 1 <= R <= 64, all with one source mode: the outgoing relations
 * of the batch's mode, in relations[mode] order) and B source rows, in ONE launch. The CSR arrays, rel_src_mode_host,
 * rel_dst_mode_host and mode_rows_host are mpqe_kg_sample_queries'. rows [B] int64 (device): the source rows; a negative row
 * is the null node. Outputs neigh [R, B, max_keep] int64 and counts [R, B] int32. Per (i, b), with len the length of row
 * rows[b]'s list in relation use_rels_host[i]:
 *   len == 0 or the null node: counts 0, every slot -1.
 *   otherwise k = min((int)ceil((double)len * keep_prob), max_keep) -- the reference's expression in the same IEEE double
 *     arithmetic -- and counts = k. k == len: the list in CSR order, no draw. k < len: the list's entries at positions
 *     P[0], .., P[k - 1] in that order, P the bijection of [0, len) that mpqe_kg_sample_rows defines, keyed by
 *     base = M[seed ^ M[slot]], slot = use_rels_host[i] << 32 | b (the relation's index in the INDEX, so a draw does not depend
 *     on which other relations the call names). Slots from k on are -1.
 * The draw is per batch POSITION: a row listed twice draws twice, like the reference. The stream is the library's, not
 * Python's (as with mpqe_sample_negatives), and the sample is over list POSITIONS: an index built with repeated edges can
 * return one neighbour twice where the reference's set would merge them.
 * A source row at or above its mode's rows, or a corrupt offset: MPQE_FLAG_BAD_INDEX, counts 0, slots -1. A neighbour outside
 * its mode: MPQE_FLAG_BAD_INDEX, that slot is -1 (counts stays k). 0 < keep_prob <= 1, 1 <= max_keep <= MPQE_SAGE_MAX_KEEP, B <=
 * 2^30 (MPQE_ERR_INVALID_ARG otherwise). B == 0: nothing is launched. No alignment beyond the element types'. */
#define MPQE_SAGE_MAX_KEEP 32
#define MPQE_SAGE_MAX_RELS 64
int mpqe_kg_sample_neighbours(const int64_t *const *rel_offsets_host, const int64_t *const *rel_rows_host,
                              const int64_t *rel_edges_host, const int32_t *rel_src_mode_host, const int32_t *rel_dst_mode_host,
                              int num_rels, const int64_t *mode_rows_host, int num_modes, const int32_t *use_rels_host /*[R]*/,
                              int R, const int64_t *rows /*[B] device*/, int64_t B, double keep_prob, int max_keep,
                              uint64_t seed, int64_t *neigh /*[R, B, max_keep]*/, int32_t *counts /*[R, B]*/, int32_t *err,
                              void *stream);

/* mpqe_sage_fwd: Encoder.forward (encoders.py:100-129) for a batch of B nodes of one mode, GIVEN the sampled neighbours, in
 * ONE launch. The mode's compress matrix W [dim_out, (R + 1) dim_in] has R + 1 column blocks, one per outgoing relation and
 * one for the node itself (R = num_rels, 0 .. MPQE_SAGE_MAX_RELS):
 *   feat_r[b] = (1 / count) * sum over s < count = counts[r, b], in slot order, of src_r[neigh[r, b, s]]          (r < R)
 *               count == 0: src_r[pad row of block r] -- the reference's single null neighbour, encoders.py:115-118
 *   feat_R[b] = src_R[self_rows[b]]                          (a negative self row: the pad row of block R)
 *   z[b]      = W . concat(feat_0 .. feat_R)                 (fp32 MFMA; the sum over k in a fixed order)
 *   out[b]    = ReLU(z)   or, with gamma and beta,   ReLU(gamma * (z - mean) / (unbiased std + eps) + beta)
 * (encoders.py:126-128, 143-146; the arithmetic of mpqe_layernorm_relu_fwd). gamma == beta == NULL: no normalisation; one
 * of them NULL: MPQE_ERR_INVALID_ARG. The rows are NOT L2-normalised: the reference's Encoder does not, only DirectEncoder.
 * Sources are named like mpqe_gqe_fwd's tables: tables_host [num_tables <= 65] with table_rows_host, any [rows, dim_in] float
 * matrix (an embedding table at depth 1, an inner encoder's output with positions as rows at depth >= 2); block r reads
 * table block_table_host[r] and its null row is block_pad_host[r] (inside the table: MPQE_ERR_INVALID_ARG otherwise). Two
 * blocks may name one table: they then share ONE gradient. The means are formed while the A operand is staged in LDS; the
 * concatenation is never written, except that with save_states != 0 the [B, (R + 1) dim_in] feature rows, z and the
 * normalisation's {mean, 1 / (std + eps)} go to `workspace` for mpqe_sage_bwd (save_states == 0: the workspace is not
 * touched and may be NULL).
 * A neighbour or self row at or above its table's rows, a negative neighbour row in a used slot, or a count outside
 * [0, max_keep] (taken as 0) ORs MPQE_FLAG_BAD_INDEX; such a row reads as zeros.
 * dim_in, dim_out: multiples of 16 up to 256 (MPQE_ERR_UNSUPPORTED otherwise, as is R * B * max_keep + B >= 2^31). Tables, W,
 * out, grad_out, grad_W and the table gradients are 16-byte aligned and the workspace 256-byte aligned, as in mpqe_gqe_fwd
 * (MPQE_ERR_INVALID_ARG otherwise); neigh, counts, self_rows, gamma, beta, grad_gamma and grad_beta take their element type's
 * alignment. B == 0: nothing is launched.
 * workspace: mpqe_sage_workspace_bytes (forward states and the backward's scratch: one size for both calls).
 *
 * mpqe_sage_bwd (the forward's arguments and workspace, its `out`, and grad_out [B, dim_out]):
 *   grad_W [dim_out, (R + 1) dim_in] += grad_z^T . feat on mpqe_linear_bwd's fixed-order tiles;
 *   grad_gamma / grad_beta [dim_out] += the ordered column sums of mpqe_layernorm_relu_bwd;
 *   grad_tables_host[t] [rows, dim_in] += per touched row the sum of its entries in entry order, one writer per row. The
 *     entries, in order: for r < R, b, s: g_feat_r[b] / count for every used slot (count == 0: g_feat_r[b] for the pad row, at
 *     s = 0); then g_feat_R[b] for the self rows. The pad row receives its gradient like any row. A stable radix sort of the
 *     (table, row) keys groups them (csrc/radix_sort.h); rows that the forward flagged get nothing.
 * NULL gradient pointers (and NULL entries of grad_tables_host) are not computed. The number of launches depends on the
 * tables' sizes (the sort's passes), not on R or B. */
size_t mpqe_sage_workspace_bytes(int64_t batch, int num_rels, int64_t dim_in, int64_t dim_out, int max_keep);
int mpqe_sage_fwd(const float *const *tables_host, const int64_t *table_rows_host, int num_tables,
                  const int32_t *block_table_host /*[R + 1]*/, const int64_t *block_pad_host /*[R + 1]*/, int num_rels,
                  const int64_t *neigh /*[R, B, max_keep]*/, const int32_t *counts /*[R, B]*/, int max_keep,
                  const int64_t *self_rows /*[B]*/, int64_t batch, const float *W, int64_t dim_in, int64_t dim_out,
                  const float *gamma, const float *beta, float eps, int save_states, float *out /*[B, dim_out]*/,
                  void *workspace, size_t workspace_bytes, int32_t *err, void *stream);
int mpqe_sage_bwd(const float *const *tables_host, const int64_t *table_rows_host, int num_tables,
                  const int32_t *block_table_host, const int64_t *block_pad_host, int num_rels, const int64_t *neigh,
                  const int32_t *counts, int max_keep, const int64_t *self_rows, int64_t batch, const float *W, int64_t dim_in,
                  int64_t dim_out, const float *gamma, const float *beta, float eps, const float *out, const float *grad_out,
                  float *const *grad_tables_host, float *grad_W, float *grad_gamma, float *grad_beta, void *workspace,
                  size_t workspace_bytes, int32_t *err, void *stream);

/* The aggregate of the intersection on its own (decoders.py:293-298, 313-318: torch.stack + agg_func(dim = 0)): out[i] =
 * mean (agg 0) / min (agg 1) of x0[i], x1[i] and, unless NULL, x2[i]; count elements. Backward: the mean's gradient in equal
 * parts, the minimum's to the first branch that holds it; NULL gradient pointers are not written. */
int mpqe_branch_agg_fwd(const float *x0, const float *x1, const float *x2, int64_t count, int agg, float *out, void *stream);
int mpqe_branch_agg_bwd(const float *x0, const float *x1, const float *x2, int64_t count, int agg, const float *grad_out,
                        float *grad_x0, float *grad_x1, float *grad_x2, void *stream);

/* ---- the evaluation metrics on device scores (csrc/eval.hip) -- added under ABI 7: entries only ---------------------------
 * reference: eval_auc_queries / eval_perc_queries utils.py:34-95 and _get_perc_scores utils.py:25-32. Integer work only
 * (comparisons, counts, a sort of 32-bit keys, integer sums): a call gives the same bits every run. Arguments are checked
 * before any launch.
 *
 * mpqe_eval_counts: scores [B + total] fp32 in forward()'s layout -- B target scores, then the negatives' scores in CSR
 * order -- and neg_offsets [B + 1] int64. counts [2, B] int64: counts[0][i] = the negatives of query i that score < its
 * target, counts[1][i] = those that score <= it (utils.py:25-32 hands scipy.stats.percentileofscore exactly these two;
 * the percentile is (lt + le + (le > lt)) * 50.0 / n in float64, NaN for n = 0). The comparisons are plain IEEE: NaN is
 * neither below nor equal on either side, -0.0 equals +0.0, a negative that IS the target ties with it.
 * A query whose offsets are out of order or outside [0, total] ORs MPQE_FLAG_BAD_INDEX into err and its two counts are
 * NOT written; the others are. B, total < 2^31 (MPQE_ERR_UNSUPPORTED above). B == 0: nothing is launched. No alignment
 * beyond the element types'. */
int mpqe_eval_counts(const float *scores, const int64_t *neg_offsets, int64_t B, int64_t total, int64_t *counts /*[2, B]*/,
                     int32_t *err, void *stream);

/* mpqe_eval_auc: the exact ROC-AUC statistic of pos [n_pos] against neg [n_neg] (the roc_auc_score call of utils.py:60-68,
 * one label per array): *u2 = sum over positives p of 2 |{neg < p}| + |{neg == p}|, so that AUC = u2 / (2 n_pos n_neg) is ONE
 * float64 division of integers. Scores compare as np.nan_to_num and == leave them on the host path: NaN counts as 0.0,
 * -0.0 as +0.0, +-inf are the extremes and tie among themselves. The negatives' order-preserving 32-bit keys are sorted with
 * the library's radix sort (csrc/radix_sort.h), every positive binary-searches its two bounds, the workgroups' integer sums
 * are added with integer atomics (order-free). n_pos == 0 or n_neg == 0: MPQE_ERR_INVALID_ARG (one class only: the AUC is
 * not defined); n_pos, n_neg < 2^31 (MPQE_ERR_UNSUPPORTED above). u2: 8-byte aligned; workspace: 4-byte aligned,
 * mpqe_eval_auc_workspace_bytes (exact: a byte less is MPQE_ERR_WORKSPACE and nothing is written; 0: arguments out of
 * range). pos and neg are only read. */
size_t mpqe_eval_auc_workspace_bytes(int64_t n_pos, int64_t n_neg);
int mpqe_eval_auc(const float *pos, int64_t n_pos, const float *neg, int64_t n_neg, uint64_t *u2, void *workspace,
                  size_t workspace_bytes, void *stream);

/* mpqe_eval_auc_segments: mpqe_eval_auc's statistic of S = num_segments slices in one call, without a host read (the
 * per-formula AUCs of an evaluation; added under ABI 7: entries only). pos_off / neg_off [S + 1] int64 on the device, CSR:
 * u2[s] is exactly what mpqe_eval_auc gives for pos[pos_off[s] .. pos_off[s + 1]) against neg[neg_off[s] .. neg_off[s + 1])
 * -- the same reading of NaN, -0.0 and +-inf --, and 0 where either slice is empty (n_pos == 0 or n_neg == 0 included).
 * The negatives' keys carry their segment above the 32-bit score key and are sorted once; a positive searches inside its
 * own segment's bounds, so equal scores of neighbouring segments are never counted. A segment whose offsets are out of
 * order or outside the arrays stays 0; nothing is read or written out of bounds. n_pos, n_neg, S < 2^31. u2 [S]: 8-byte
 * aligned; workspace: 8-byte aligned, mpqe_eval_auc_segments_workspace_bytes (exact: a byte less is MPQE_ERR_WORKSPACE and
 * nothing is written; 0: arguments out of range). */
size_t mpqe_eval_auc_segments_workspace_bytes(int64_t n_pos, int64_t n_neg, int64_t num_segments);
int mpqe_eval_auc_segments(const float *pos, int64_t n_pos, const float *neg, int64_t n_neg, const int64_t *pos_off,
                           const int64_t *neg_off, int64_t num_segments, uint64_t *u2 /*[num_segments]*/, void *workspace,
                           size_t workspace_bytes, void *stream);

/* Diagnostics, not part of the data path: while `device_buffer` (8 int64 per workgroup, num_blocks
 * workgroups) is set, every chain-kernel launch with at most num_blocks workgroups writes per workgroup the
 * device wall clock (100 MHz) at its phase boundaries [0..6] and HW_ID | XCC_ID << 32 in [7]; workgroup g of a
 * launch of G workgroups also writes its shader-clock ticks at the first / last stamp to words 0 / 1 of entry
 * G + g, so 2 G <= num_blocks is required. NULL turns it off. Process-global; tools/chain_timeline.py only. */
void mpqe_debug_chain_stamps(void *device_buffer, size_t num_blocks);
/* The same for the weight-gradient launch: 8 int64 per workgroup: wall clock at start [0] and end [1], shader-clock
 * ticks start -> end [2], HW_ID | XCC_ID << 32 in [3], wall clock when the tile's record is read [4], when its first
 * K-step has landed [5] and when its K loop ends [6].                                                */
void mpqe_debug_tail_stamps(void *device_buffer, size_t num_blocks);
/* Named diagnostics switches (timing experiments; tests that force a rarely taken path, e.g. "TOUCH_MULTI_LAUNCH" = the
 * multi-launch sort (csrc/radix_sort.h) instead of the one-launch sort, "TSORT_FAIL" = the in-step sort gives up as if its workgroups were not
 * co-resident, "GEN_SLOTS" = grid size of the persistent gather-GEMMs, "PROLOGUE_LAST" = 1 / 0: the chain launch's prologue
 * items behind / in front of its chain workgroups whatever their number, "NO_RUNS" = the reduction's table workgroups take
 * every sorted position of the touch plan instead of its compacted run starts, "DUMP_PLAN" = the step's plan and launch shape
 * on stderr). set != 0 stores `value` under `name`, set == 0 removes it. Process-global (see Conventions).      */
void mpqe_debug_option(const char *name, int value, int set);

#ifdef __cplusplus
}
#endif
#endif /* MPQE_AMD_H */
