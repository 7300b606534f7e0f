// R-GCN layer over a batch of B replicas of ONE query template (row = b*N + n).
// reference: RGCNConv.forward/message/update, mpqe/model.py:269-305, applied to
// the Batch built by data_utils.py:394-405.
//
// Because every graph shares the template, the neighbour aggregation is not a
// scatter at all: for node slot n with in-edges e1..ek
//     out[:, n, :] = [x[:, src_e1, :] | ... | x[:, src_ek, :] | x[:, n, :]]
//                    . [basis[r_e1]; ...; basis[r_ek]; root]  + bias
// i.e. a GEMM whose K dimension is the concatenation over incoming edges, so the
// sum over neighbours happens inside the MFMA accumulator. bias and ReLU are
// fused into the epilogue. Backward-x is the same on the reversed template with
// W^T; the weight gradient is x_src^T . g_dst with the batch as K, split over
// workgroups and reduced in a fixed order (no float atomics -> reproducible).
#include "bias_grad.h"
#include "rgcn_template_body.h"

// ------------------------------------------------------------------------------------ forward
template <int MODE>
__global__ __launch_bounds__(256) void rgcn_tmpl_fwd_kernel(
    TmplArgs tp, long long B, const float *__restrict__ x, const float *__restrict__ basis,
    const float *__restrict__ root, const float *__restrict__ bias, int Din, int Dout, int relu,
    float *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) float smem[GT_SMEM_FLOATS];
    tmpl_fwd_tile<MODE>(tp, B, x, basis, root, bias, Din, Dout, relu, out, (int)blockIdx.z,
                       (long long)blockIdx.x * GT_BM, (int)blockIdx.y * GT_BN, smem);
}

// ------------------------------------------------------------------------------------ backward wrt x
template <int MODE>
__global__ __launch_bounds__(256) void rgcn_tmpl_bwd_x_kernel(
    TmplArgs tp, long long B, const float *__restrict__ g, const float *__restrict__ out,
    const float *__restrict__ basis, const float *__restrict__ root, int Din, int Dout, int relu,
    float *__restrict__ grad_x) {
    __shared__ __attribute__((aligned(16))) float smem[GT_SMEM_FLOATS];
    tmpl_bwd_x_tile<MODE>(tp, B, g, out, basis, root, Din, Dout, relu, grad_x, (int)blockIdx.z,
                         (long long)blockIdx.x * GT_BM, (int)blockIdx.y * GT_BN, smem);
}

// ------------------------------------------------------------------------------------ weight gradient
// slot z < E : slab = sum_{b in chunk} x[b*N+src_z]^T (x) gpre[b*N+dst_z]      (-> basis[rel_z])
// slot z = E : slab = sum_{q in chunk} x[q]^T (x) gpre[q], q over all B*N rows  (-> root)
// One workgroup = one 64x64 tile of one K-chunk; slabs go to the workspace and are summed
// in fixed order by rgcn_tmpl_reduce_w_kernel.
struct WChunks {
    int nch_edge, ch_edge;     // chunks per edge slot, rows per chunk
    int nch_root, ch_root;
};

template <int MODE>
__global__ __launch_bounds__(256) void rgcn_tmpl_grad_w_kernel(
    TmplArgs tp, WChunks wc, long long B, const float *__restrict__ x, const float *__restrict__ g,
    const float *__restrict__ out, int Din, int Dout, int relu, float *__restrict__ slabs) {
    __shared__ __attribute__((aligned(16))) float smem[GT_SMEM_FLOATS];
    const int z = blockIdx.z;
    const int c = blockIdx.x;
    const bool is_root = (z == tp.E);
    const int nch = is_root ? wc.nch_root : wc.nch_edge;
    if (c >= nch) return;
    const int tiles_j = (Dout + GT_BN - 1) / GT_BN;
    const int i0 = (blockIdx.y / tiles_j) * GT_BM;
    const int j0 = (blockIdx.y % tiles_j) * GT_BN;
    const long long count = is_root ? B * tp.N : B;
    const long long ch = is_root ? wc.ch_root : wc.ch_edge;
    const long long q0 = (long long)c * ch;
    long long q1 = q0 + ch;
    if (q1 > count) q1 = count;
    const long long xs = is_root ? 1 : tp.N, xo = is_root ? 0 : tp.src[z];
    const long long gs = is_root ? 1 : tp.N, go = is_root ? 0 : tp.dst[z];
    const long long slab = is_root ? (long long)tp.E * wc.nch_edge + c : (long long)z * wc.nch_edge + c;
    tmpl_grad_w_tile<MODE>(x, g, out, Din, Dout, relu, xs, xo, gs, go, q0, q1, i0, j0,
                          slabs + slab * (long long)Din * Dout, smem);
}

// grad_basis[rel_z] += sum over (slots sharing rel_z, chunks) in fixed order; grad_root likewise.
__global__ __launch_bounds__(256) void rgcn_tmpl_reduce_w_kernel(
    TmplArgs tp, WChunks wc, int Din, int Dout, const float *__restrict__ slabs,
    float *__restrict__ grad_basis, float *__restrict__ grad_root) {
    const int z = blockIdx.y;
    const long long elems = (long long)Din * Dout;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= elems) return;
    if (z == tp.E) {
        if (!grad_root) return;
        float s = 0.f;
        const float *p = slabs + (long long)tp.E * wc.nch_edge * elems + idx;
        for (int c = 0; c < wc.nch_root; ++c) s += p[(long long)c * elems];
        grad_root[idx] += s;
        return;
    }
    if (!grad_basis) return;
    for (int zz = 0; zz < z; ++zz)
        if (tp.rel[zz] == tp.rel[z]) return;          // an earlier slot owns this relation
    float s = 0.f;
    for (int zz = z; zz < tp.E; ++zz) {
        if (tp.rel[zz] != tp.rel[z]) continue;
        const float *p = slabs + (long long)zz * wc.nch_edge * elems + idx;
        for (int c = 0; c < wc.nch_edge; ++c) s += p[(long long)c * elems];
    }
    grad_basis[tp.rel[z] * elems + idx] += s;
}

// ------------------------------------------------------------------------------------ host side
static int fill_tmpl(int query_type, const int64_t *edge_type_host, int64_t num_relations, TmplArgs *tp) {
    if (query_type < 0 || query_type >= MPQE_Q_COUNT || !edge_type_host) return MPQE_ERR_INVALID_ARG;
    const TemplateDesc &d = kTemplates[query_type];
    tp->N = d.N;
    tp->E = d.E;
    for (int e = 0; e < 3; ++e) {
        tp->src[e] = e < d.E ? d.src[e] : 0;
        tp->dst[e] = e < d.E ? d.dst[e] : 0;
        tp->rel[e] = e < d.E ? edge_type_host[e] : 0;
        if (e < d.E && (edge_type_host[e] < 0 || edge_type_host[e] >= num_relations))
            return MPQE_ERR_INVALID_ARG;
    }
    return MPQE_OK;
}

static WChunks plan_chunks(int64_t B, int N) {
    auto pick = [](int64_t count, int max_chunks, int *nch, int *ch) {
        int64_t n = (count + 127) / 128;
        if (n < 1) n = 1;
        if (n > max_chunks) n = max_chunks;
        int64_t c = (count + n - 1) / n;
        c = (c + GT_BK - 1) / GT_BK * GT_BK;
        if (c < GT_BK) c = GT_BK;
        n = (count + c - 1) / c;
        if (n < 1) n = 1;
        *nch = (int)n;
        *ch = (int)c;
    };
    WChunks w;
    pick(B, 16, &w.nch_edge, &w.ch_edge);
    pick(B * N, 32, &w.nch_root, &w.ch_root);
    return w;
}

extern "C" int mpqe_template_info(int query_type, mpqe_template_t *o) {
    if (query_type < 0 || query_type >= MPQE_Q_COUNT || !o) return MPQE_ERR_INVALID_ARG;
    const TemplateDesc &d = kTemplates[query_type];
    o->num_anchors = d.A;
    o->num_vars = d.V;
    o->num_nodes = d.N;
    o->num_edges = d.E;
    o->diameter = d.diam;
    for (int e = 0; e < 3; ++e) {
        o->src[e] = d.src[e];
        o->dst[e] = d.dst[e];
        o->rel_label[e] = d.rel_label[e];
    }
    for (int v = 0; v < 4; ++v) o->var_node[v] = d.var_node[v];
    return MPQE_OK;
}

extern "C" int mpqe_rgcn_template_fwd(int query_type, int64_t B, const int64_t *edge_type_host,
                                      const float *x, const float *basis, int64_t R, const float *root,
                                      const float *bias, int64_t Din, int64_t Dout, int relu, float *out,
                                      void *stream) {
    TmplArgs tp;
    int st = fill_tmpl(query_type, edge_type_host, R, &tp);
    if (st) return st;
    if (!x || !basis || !root || !out || B < 0 || Din <= 0 || Dout <= 0) return MPQE_ERR_INVALID_ARG;
    if (Din > (1 << 20) || Dout > (1 << 20)) return MPQE_ERR_UNSUPPORTED;
    if (B == 0) return MPQE_OK;
    dim3 grid((unsigned)((B + GT_BM - 1) / GT_BM), (unsigned)((Dout + GT_BN - 1) / GT_BN), tp.N);
    // one compile-time switch: every operand row is 16-byte aligned (dims % 4 == 0) or none is assumed to be
    const bool vec = ptr_vec_ok(x, Din) && ptr_vec_ok(basis, Dout) && ptr_vec_ok(root, Dout) && (Din * Dout) % 4 == 0;
    const bool fast = vec && Din % GT_BK == 0 && Dout % GT_BN == 0;
    if (fast)
        hipLaunchKernelGGL(rgcn_tmpl_fwd_kernel<LD_FAST>, grid, dim3(256), 0, as_stream(stream), tp, (long long)B,
                           x, basis, root, bias, (int)Din, (int)Dout, relu, out);
    else if (vec)
        hipLaunchKernelGGL(rgcn_tmpl_fwd_kernel<LD_PRED>, grid, dim3(256), 0, as_stream(stream), tp, (long long)B,
                           x, basis, root, bias, (int)Din, (int)Dout, relu, out);
    else
        hipLaunchKernelGGL(rgcn_tmpl_fwd_kernel<LD_SCALAR>, grid, dim3(256), 0, as_stream(stream), tp,
                           (long long)B, x, basis, root, bias, (int)Din, (int)Dout, relu, out);
    return mpqe_launch_status();
}

static size_t tmpl_slab_floats(const TmplArgs &tp, const WChunks &w, int64_t Din, int64_t Dout) {
    return (size_t)(tp.E * w.nch_edge + w.nch_root) * (size_t)Din * (size_t)Dout;
}

extern "C" size_t mpqe_rgcn_template_bwd_workspace_bytes(int query_type, int64_t B, int64_t Din, int64_t Dout) {
    if (query_type < 0 || query_type >= MPQE_Q_COUNT || B < 0) return 0;
    const TemplateDesc &d = kTemplates[query_type];
    TmplArgs tp;
    tp.N = d.N;
    tp.E = d.E;
    WChunks w = plan_chunks(B, d.N);
    return align_up(tmpl_slab_floats(tp, w, Din, Dout) * 4, 256) + bias_partial_bytes((long long)B * d.N, Dout) + 256;
}

extern "C" int mpqe_rgcn_template_bwd(int query_type, int64_t B, const int64_t *edge_type_host, const float *x,
                                      const float *out, const float *grad_out, const float *basis, int64_t R,
                                      const float *root, int64_t Din, int64_t Dout, int relu, float *grad_x,
                                      float *grad_basis, float *grad_root, float *grad_bias, void *workspace,
                                      size_t workspace_bytes, void *stream) {
    TmplArgs tp;
    int st = fill_tmpl(query_type, edge_type_host, R, &tp);
    if (st) return st;
    if (!x || !grad_out || !basis || !root || B < 0 || Din <= 0 || Dout <= 0) return MPQE_ERR_INVALID_ARG;
    if (relu && !out) return MPQE_ERR_INVALID_ARG;
    if (B == 0) return MPQE_OK;
    // (refused before anything is queued: a short workspace must not leave grad_x written behind an error)
    if ((grad_basis || grad_root || grad_bias) &&
        (workspace_bytes < mpqe_rgcn_template_bwd_workspace_bytes(query_type, B, Din, Dout) || !workspace))
        return MPQE_ERR_WORKSPACE;
    // (the bias sums pick their 16-byte form by the workspace's address too: the result's bits must not hang on it)
    if ((grad_basis || grad_root || grad_bias) && (uintptr_t)workspace % 16 != 0) return MPQE_ERR_INVALID_ARG;
    hipStream_t s = as_stream(stream);
    const bool vec = ptr_vec_ok(basis, Dout) && ptr_vec_ok(root, Dout) && (Din * Dout) % 4 == 0 &&
                     ptr_vec_ok(grad_out, Dout) && (!relu || ptr_vec_ok(out, Dout)) && ptr_vec_ok(x, Din);
    if (grad_x) {
        dim3 grid((unsigned)((B + GT_BM - 1) / GT_BM), (unsigned)((Din + GT_BN - 1) / GT_BN), tp.N);
        if (vec && Dout % GT_BK == 0 && Din % GT_BN == 0)
            hipLaunchKernelGGL(rgcn_tmpl_bwd_x_kernel<LD_FAST>, grid, dim3(256), 0, s, tp, (long long)B, grad_out,
                               out, basis, root, (int)Din, (int)Dout, relu, grad_x);
        else if (vec)
            hipLaunchKernelGGL(rgcn_tmpl_bwd_x_kernel<LD_PRED>, grid, dim3(256), 0, s, tp, (long long)B, grad_out,
                               out, basis, root, (int)Din, (int)Dout, relu, grad_x);
        else
            hipLaunchKernelGGL(rgcn_tmpl_bwd_x_kernel<LD_SCALAR>, grid, dim3(256), 0, s, tp, (long long)B, grad_out,
                               out, basis, root, (int)Din, (int)Dout, relu, grad_x);
    }
    if (grad_basis || grad_root || grad_bias) {
        WChunks w = plan_chunks(B, tp.N);
        float *slabs = reinterpret_cast<float *>(workspace);
        float *bias_part = reinterpret_cast<float *>(reinterpret_cast<char *>(workspace) +
                                                     align_up(tmpl_slab_floats(tp, w, Din, Dout) * 4, 256));
        if (grad_basis || grad_root) {
            const int tiles = (int)(((Din + GT_BM - 1) / GT_BM) * ((Dout + GT_BN - 1) / GT_BN));
            const int maxch = w.nch_root > w.nch_edge ? w.nch_root : w.nch_edge;
            dim3 grid(maxch, tiles, tp.E + 1);
            // LD_FAST needs whole K-steps in every chunk (the K dimension is the batch here)
            if (vec && Din % GT_BM == 0 && Dout % GT_BN == 0 && B % GT_BK == 0)
                hipLaunchKernelGGL(rgcn_tmpl_grad_w_kernel<LD_FAST>, grid, dim3(256), 0, s, tp, w, (long long)B, x,
                                   grad_out, out, (int)Din, (int)Dout, relu, slabs);
            else if (vec)
                hipLaunchKernelGGL(rgcn_tmpl_grad_w_kernel<LD_PRED>, grid, dim3(256), 0, s, tp, w, (long long)B, x,
                                   grad_out, out, (int)Din, (int)Dout, relu, slabs);
            else
                hipLaunchKernelGGL(rgcn_tmpl_grad_w_kernel<LD_SCALAR>, grid, dim3(256), 0, s, tp, w, (long long)B,
                                   x, grad_out, out, (int)Din, (int)Dout, relu, slabs);
            const long long elems = (long long)Din * Dout;
            dim3 rgrid((unsigned)((elems + 255) / 256), tp.E + 1);
            hipLaunchKernelGGL(rgcn_tmpl_reduce_w_kernel, rgrid, dim3(256), 0, s, tp, w, (int)Din, (int)Dout,
                               slabs, grad_basis, grad_root);
        }
        if (grad_bias) {
            launch_bias_grad((long long)B * tp.N, grad_out, out, (int)Dout, relu, bias_part, grad_bias, s);
        }
    }
    return mpqe_launch_status();
}
