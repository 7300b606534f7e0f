"""torch.autograd bindings of the C ABI (include/mpqe_amd.h). PyTorch here is plumbing:
device memory (caching allocator), the current HIP stream and autograd bookkeeping. All
arithmetic runs in the gfx950 kernels; tensors must be CUDA fp32/int64 and contiguous,
anything else raises -- there is no CPU or eager-PyTorch path.
"""
import contextlib

import numpy as np
import torch

from . import _capi, _lib
from ._capi import QUERY_TYPE_IDS, READOUT_IDS, SCATTER_IDS


def lib():
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _need(t, dtype, what):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError('mpqe_amd: %s must be a CUDA (ROCm) tensor -- there is no CPU path' % what)
    if t.dtype != dtype:
        raise TypeError('mpqe_amd: %s must be %s, got %s' % (what, dtype, t.dtype))
    return t if t.is_contiguous() else t.contiguous()


def _f(t, what):
    return _need(t, torch.float32, what)


def _i(t, what):
    return _need(t, torch.int64, what)


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def _ck(st, what):
    _capi.check(lib(), st, what)


def new_error_word(device):
    return torch.zeros(1, dtype=torch.int32, device=device)


flag_clears = 0       # how often the host has rewritten a non-zero error word (clear_flags): FlatOptimizer(guard=True) re-reads
                      # its device count of applied updates when this has moved -- updates may have been refused meanwhile


def clear_flags(err, value=0):
    """Rewrite an error word the host has read as non-zero (value: the bits that stay). Every such site goes through here."""
    global flag_clears
    err.fill_(value)
    flag_clears += 1


def raise_on_flags(err):
    """One 4-byte D2H read (synchronises). Mirrors the IndexError the reference's
    index_select / nn.Embedding raise on a bad id."""
    flags = int(err.item())
    if flags:
        clear_flags(err)
        names = [n for bit, n in ((1, 'entity id outside node_map / not of this mode'),
                                  (2, 'edge endpoint outside [0, num_nodes)'),
                                  (4, 'edge type outside [0, num_relations)'),
                                  (8, 'scatter index outside [0, dim_size)')) if flags & bit]
        if flags & 16:
            sites = [n for bit, n in ((0x100, 'a pre-pass vector'), (0x200, 'the transposed weight copies'),
                                      (0x400, 'a completion counter'), (0x800, 'a vector op\'s inputs'),
                                      (0x2000, 'the touch plan\'s sort'),
                                      (0x4000, 'a peer of the p2p gradient exchange')) if flags & bit]
            raise RuntimeError('mpqe_amd: an in-launch hand-off between workgroups timed out (library fault): '
                               + (', '.join(sites) or 'unknown site'))
        if flags & 32:
            raise RuntimeError('mpqe_amd: a step could not build its own touch plan (the sort\'s workgroups were not all '
                               'resident at once -- a shared GPU?) and its entity-table gradients were NOT accumulated; '
                               'FusedTrainStep.run(..., checked=True) rebuilds the plan and recovers them')
        raise IndexError('mpqe_amd: ' + '; '.join(names))


# --------------------------------------------------------------------------------------------- templates
class Template(object):
    """Host-side description of a batch of B replicas of one query template."""
    __slots__ = ('query_type', 'qid', 'B', 'N', 'E', 'A', 'V', 'diameter', 'edge_type', '_et')

    def __init__(self, query_type, batch_size, edge_type):
        if query_type not in QUERY_TYPE_IDS:
            raise ValueError('unknown query type %r' % (query_type,))
        info = _capi.TemplateInfo()
        _ck(lib().mpqe_template_info(QUERY_TYPE_IDS[query_type], info), 'mpqe_template_info')
        self.query_type = query_type
        self.qid = QUERY_TYPE_IDS[query_type]
        self.B = int(batch_size)
        self.N, self.E = info.num_nodes, info.num_edges
        self.A, self.V = info.num_anchors, info.num_vars
        self.diameter = info.diameter
        self.edge_type = tuple(int(e) for e in edge_type)
        if len(self.edge_type) != self.E:
            raise ValueError('%s has %d edges, got %d edge types' % (query_type, self.E, len(self.edge_type)))
        self._et = np.ascontiguousarray(np.array(self.edge_type, dtype=np.int64))

    @property
    def et_ptr(self):
        return self._et.ctypes.data


def template_info(query_type):
    info = _capi.TemplateInfo()
    _ck(lib().mpqe_template_info(QUERY_TYPE_IDS[query_type], info), 'mpqe_template_info')
    return info


def collate_template(tmpl, device):
    """(a1) device-side expansion of the template: edge_index [2,B*E], edge_type [B*E], batch [B*N]."""
    ei = torch.empty((2, tmpl.B * tmpl.E), dtype=torch.int64, device=device)
    et = torch.empty((tmpl.B * tmpl.E,), dtype=torch.int64, device=device)
    bt = torch.empty((tmpl.B * tmpl.N,), dtype=torch.int64, device=device)
    with torch.cuda.device(device):
        _ck(lib().mpqe_collate_template(tmpl.qid, tmpl.B, tmpl.et_ptr, _p(ei), _p(et), _p(bt), _stream()),
            'mpqe_collate_template')
    return ei, et, bt


# --------------------------------------------------------------------------------------------- general-graph plan
class GraphPlan(object):
    """Sorted views of an arbitrary edge list (by relation / destination / source), built once
    per graph on the device. Raises IndexError for out-of-range endpoints or edge types."""

    def __init__(self, edge_index, edge_type, num_nodes, num_relations):
        edge_index = _i(edge_index, 'edge_index')
        edge_type = _i(edge_type, 'edge_type')
        if edge_index.dim() != 2 or edge_index.shape[0] != 2 or edge_type.shape[0] != edge_index.shape[1]:
            raise ValueError('edge_index must be [2, E] and edge_type [E]')
        self.Nn, self.E, self.R = int(num_nodes), int(edge_index.shape[1]), int(num_relations)
        L = lib()
        dev = edge_index.device
        with torch.cuda.device(dev):
            pb = L.mpqe_rgcn_plan_bytes(self.Nn, self.E, self.R)
            pw = L.mpqe_rgcn_plan_workspace_bytes(self.Nn, self.E, self.R)
            self.buf = _ws(pb, dev)
            ws = _ws(pw, dev)
            err = new_error_word(dev)
            _ck(L.mpqe_rgcn_plan_build(_p(edge_index), _p(edge_type), self.Nn, self.E, self.R, _p(self.buf), pb,
                                       _p(ws), pw, _p(err), _stream()), 'mpqe_rgcn_plan_build')
            raise_on_flags(err)


# --------------------------------------------------------------------------------------------- R-GCN layer
class _RGCNLayer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, basis, root, bias, graph, relu):
        x, basis, root = _f(x, 'x'), _f(basis, 'basis'), _f(root, 'root')
        bias = None if bias is None else _f(bias, 'bias')
        R, Din, Dout = basis.shape
        if x.dim() != 2 or x.shape[1] != Din or tuple(root.shape) != (Din, Dout):
            raise ValueError('shape mismatch: x %s basis %s root %s' % (tuple(x.shape), tuple(basis.shape),
                                                                        tuple(root.shape)))
        L = lib()
        out = torch.empty((x.shape[0], Dout), dtype=torch.float32, device=x.device)
        mask_bits = None
        with torch.cuda.device(x.device):
            if isinstance(graph, Template):
                if x.shape[0] != graph.B * graph.N:
                    raise ValueError('x has %d rows, template batch needs %d' % (x.shape[0], graph.B * graph.N))
                _ck(L.mpqe_rgcn_template_fwd(graph.qid, graph.B, graph.et_ptr, _p(x), _p(basis), R, _p(root),
                                             _p(bias), Din, Dout, int(relu), _p(out), _stream()),
                    'mpqe_rgcn_template_fwd')
            else:
                if graph.Nn != x.shape[0] or graph.R != R:
                    raise ValueError('plan was built for %d nodes / %d relations' % (graph.Nn, graph.R))
                wb = L.mpqe_rgcn_general_workspace_bytes(graph.Nn, graph.E, R, Din, Dout, 0)
                ws = _ws(wb, x.device)
                # (the ReLU mask as bit words, 1 / 32 of `out`: the backward masks with them instead of gathering `out` rows)
                mb = L.mpqe_rgcn_general_mask_bytes(graph.Nn, Dout) if relu else 0
                if mb:
                    mask_bits = torch.empty(mb // 8, dtype=torch.int64, device=x.device)
                _ck(L.mpqe_rgcn_general_fwd(_p(graph.buf), graph.Nn, graph.E, R, _p(x), _p(basis), _p(root),
                                            _p(bias), Din, Dout, int(relu), _p(out), _p(mask_bits), _p(ws), wb, _stream()),
                    'mpqe_rgcn_general_fwd')
        ctx.graph, ctx.relu, ctx.has_bias = graph, bool(relu), bias is not None
        ctx.save_for_backward(x, basis, root, out if relu else None, mask_bits)
        return out

    @staticmethod
    def backward(ctx, g):
        x, basis, root, out, mask_bits = ctx.saved_tensors
        g = _f(g, 'grad_out')
        graph, relu = ctx.graph, ctx.relu
        R, Din, Dout = basis.shape
        L = lib()
        need_x, need_b, need_r, need_bias = ctx.needs_input_grad[:4]
        gx = torch.empty_like(x) if need_x else None
        general = not isinstance(graph, Template)
        # (general graphs: the call writes every gradient buffer whole -- no zero fill, no read-modify-write)
        gb = (torch.empty_like(basis) if general else torch.zeros_like(basis)) if need_b else None
        gr = (torch.empty_like(root) if general else torch.zeros_like(root)) if need_r else None
        gbias = ((torch.empty if general else torch.zeros)(Dout, dtype=torch.float32, device=x.device)
                 if (need_bias and ctx.has_bias) else None)
        with torch.cuda.device(x.device):
            if isinstance(graph, Template):
                wb = L.mpqe_rgcn_template_bwd_workspace_bytes(graph.qid, graph.B, Din, Dout)
                ws = _ws(wb, x.device)
                _ck(L.mpqe_rgcn_template_bwd(graph.qid, graph.B, graph.et_ptr, _p(x), _p(out), _p(g), _p(basis), R,
                                             _p(root), Din, Dout, int(relu), _p(gx), _p(gb), _p(gr), _p(gbias),
                                             _p(ws), wb, _stream()), 'mpqe_rgcn_template_bwd')
            else:
                wb = L.mpqe_rgcn_general_workspace_bytes(graph.Nn, graph.E, R, Din, Dout, 1)
                ws = _ws(wb, x.device)
                _ck(L.mpqe_rgcn_general_bwd(_p(graph.buf), graph.Nn, graph.E, R, _p(x), _p(out), _p(mask_bits), _p(g), _p(basis),
                                            _p(root), Din, Dout, int(relu), 1, _p(gx), _p(gb), _p(gr), _p(gbias),
                                            _p(ws), wb, _stream()), 'mpqe_rgcn_general_bwd')
        return gx, gb, gr, gbias, None, None


def rgcn_layer(x, basis, root, bias, graph, relu=False):
    """out = [relu](sum_e x[src_e].basis[type_e] + x.root + bias); graph is a Template or a GraphPlan."""
    return _RGCNLayer.apply(x, basis, root, bias, graph, relu)


# --------------------------------------------------------------------------------------------- dense layer
class _Linear(torch.autograd.Function):
    """y = [relu](sum_k x_k . W[:, off_k : off_k + w_k]^T + bias): nn.Linear's arithmetic on the library's own MFMA tiles
    (mpqe_linear_fwd / mpqe_linear_bwd). One block = a plain dense layer; several = one wide matrix applied block by
    block to inputs that are never concatenated (Encoder.forward's compress product, reference encoders.py:120-124);
    the column blocks of W -- and of its gradient -- are read and written in place through the row stride."""

    @staticmethod
    def forward(ctx, W, bias, relu, blocks, *xs):
        W = _f(W, 'weight')
        xs = [_f(x, 'x') for x in xs]
        bias = None if bias is None else _f(bias, 'bias')
        if W.dim() != 2 or len(xs) != len(blocks) or not xs:
            raise ValueError('one column block of the weight per input')
        dout, total = W.shape
        rows = xs[0].shape[0]
        for x, (off, width) in zip(xs, blocks):
            if x.dim() != 2 or x.shape[0] != rows or x.shape[1] != width or off < 0 or off + width > total:
                raise ValueError('shape mismatch: x %s, weight block [%d, %d:%d]' % (tuple(x.shape), dout, off, off + width))
        y = torch.empty((rows, dout), dtype=torch.float32, device=W.device)
        L = lib()
        with torch.cuda.device(y.device):
            for k, (x, (off, width)) in enumerate(zip(xs, blocks)):
                last = k == len(xs) - 1
                _ck(L.mpqe_linear_fwd(_p(x), rows, W.data_ptr() + 4 * off, total, _p(bias) if last else None, width, dout,
                                      int(bool(relu) and last), int(k > 0), _p(y), _stream()), 'mpqe_linear_fwd')
        ctx.relu, ctx.blocks, ctx.has_bias = bool(relu), list(blocks), bias is not None
        ctx.save_for_backward(W, y if relu else None, *xs)
        return y

    @staticmethod
    def backward(ctx, g):
        W, y = ctx.saved_tensors[:2]
        xs = ctx.saved_tensors[2:]
        g = _f(g, 'grad_out')
        rows, dout = g.shape
        total = W.shape[1]
        L = lib()
        need_w, need_bias = ctx.needs_input_grad[0], ctx.needs_input_grad[1] and ctx.has_bias
        pos, covered = 0, True
        for o, w in sorted(ctx.blocks):
            covered, pos = covered and o == pos, o + w
        covered = covered and pos == total
        gW = ((torch.empty_like(W) if covered else torch.zeros_like(W)) if need_w else None)    # (blocks that tile W: written whole)
        gbias = torch.empty(dout, dtype=torch.float32, device=g.device) if need_bias else None
        gxs = []
        with torch.cuda.device(g.device):
            for k, (x, (off, width)) in enumerate(zip(xs, ctx.blocks)):
                gx = torch.empty_like(x) if ctx.needs_input_grad[4 + k] else None
                wb = L.mpqe_linear_bwd_workspace_bytes(rows, width, dout)
                ws = _ws(wb, g.device)
                _ck(L.mpqe_linear_bwd(_p(x), rows, W.data_ptr() + 4 * off, total, _p(y), _p(g), width, dout, int(ctx.relu), 1,
                                      _p(gx), None if gW is None else gW.data_ptr() + 4 * off, total,
                                      _p(gbias) if k == 0 else None, _p(ws), wb, _stream()), 'mpqe_linear_bwd')
                gxs.append(gx)
        return (gW, gbias, None, None) + tuple(gxs)


def linear(x, weight, bias=None, relu=False):
    """[relu](x . weight^T + bias), weight [out, in] as nn.Linear stores it."""
    return _Linear.apply(weight, bias, relu, [(0, weight.shape[1])], x)


def blocks_linear(xs, weight, blocks, bias=None, relu=False):
    """[relu](sum_k xs[k] . weight[:, off_k : off_k + w_k]^T + bias), blocks = [(off_k, w_k)]: one wide matrix applied block
    by block, the inputs never concatenated."""
    return _Linear.apply(weight, bias, relu, list(blocks), *xs)


# --------------------------------------------------------------------------------------------- embeddings
class _EmbedL2Norm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, node_map, ids, err):
        table, ids = _f(table, 'embedding table'), _i(ids, 'ids')
        node_map = None if node_map is None else _i(node_map, 'node_map')
        n, D = ids.shape[0], table.shape[1]
        out = torch.empty((n, D), dtype=torch.float32, device=table.device)
        with torch.cuda.device(table.device):
            _ck(lib().mpqe_embed_l2norm_fwd(_p(table), table.shape[0], D, _p(node_map),
                                            0 if node_map is None else node_map.shape[0], _p(ids), n, _p(out), D,
                                            None, _p(err), _stream()), 'mpqe_embed_l2norm_fwd')
        ctx.save_for_backward(table, ids)
        ctx.node_map, ctx.err = node_map, err
        return out

    @staticmethod
    def backward(ctx, g):
        table, ids = ctx.saved_tensors
        g = _f(g, 'grad')
        node_map = ctx.node_map
        gt = torch.zeros_like(table)
        with torch.cuda.device(table.device):
            _ck(lib().mpqe_embed_l2norm_bwd(_p(g), g.shape[1], _p(table), table.shape[0], table.shape[1],
                                            _p(node_map), 0 if node_map is None else node_map.shape[0], _p(ids),
                                            ids.shape[0], _p(gt), _p(ctx.err), _stream()), 'mpqe_embed_l2norm_bwd')
        return gt, None, None, None


def embed_l2norm(table, node_map, ids, err=None):
    """(a2) rows = node_map[ids]; table[rows] / ||.||_2   -> [n, D]"""
    return _EmbedL2Norm.apply(table, node_map, ids, err)


class _AssembleX(torch.autograd.Function):
    """(a3) x[b, i] = normalise(table_i[node_map[anchor_ids[i, b]]]); x[b, A+k] = mode_emb[var_ids[k]].
    anchor_ids_t is [A, B] (one contiguous id row per anchor slot)."""

    @staticmethod
    def forward(ctx, mode_emb, node_map, anchor_ids_t, var_ids, slot_table, err, *tables):
        mode_emb = _f(mode_emb, 'mode_embeddings.weight')
        anchor_ids_t, var_ids = _i(anchor_ids_t, 'anchor_ids'), _i(var_ids, 'var_ids')
        node_map = None if node_map is None else _i(node_map, 'node_map')
        tables = [_f(t, 'embedding table') for t in tables]
        A, B = anchor_ids_t.shape
        V = var_ids.shape[0]
        N, D = A + V, mode_emb.shape[1]
        L = lib()
        x = torch.empty((B * N, D), dtype=torch.float32, device=mode_emb.device)
        with torch.cuda.device(x.device):
            for i in range(A):
                t = tables[slot_table[i]]
                if t.shape[1] != D:
                    raise ValueError('embedding dim mismatch')
                _ck(L.mpqe_embed_l2norm_fwd(_p(t), t.shape[0], D, _p(node_map),
                                            0 if node_map is None else node_map.shape[0],
                                            anchor_ids_t.data_ptr() + 8 * i * B, B, x.data_ptr() + 4 * i * D,
                                            N * D, None, _p(err), _stream()), 'mpqe_embed_l2norm_fwd')
            _ck(L.mpqe_var_rows_fwd(_p(mode_emb), mode_emb.shape[0], D, _p(var_ids), V, B, N, A, _p(x), _p(err),
                                    _stream()), 'mpqe_var_rows_fwd')
        ctx.save_for_backward(mode_emb, anchor_ids_t, var_ids, *tables)
        ctx.node_map, ctx.slot_table, ctx.err = node_map, slot_table, err
        return x

    @staticmethod
    def backward(ctx, g):
        mode_emb, anchor_ids_t, var_ids = ctx.saved_tensors[:3]
        tables = ctx.saved_tensors[3:]
        g = _f(g, 'grad_x')
        node_map, err = ctx.node_map, ctx.err
        A, B = anchor_ids_t.shape
        V = var_ids.shape[0]
        N, D = A + V, mode_emb.shape[1]
        L = lib()
        gmode = torch.zeros_like(mode_emb) if ctx.needs_input_grad[0] else None
        gtabs = [torch.zeros_like(t) if ctx.needs_input_grad[6 + j] else None for j, t in enumerate(tables)]
        with torch.cuda.device(g.device):
            for i in range(A):
                j = ctx.slot_table[i]
                if gtabs[j] is None:
                    continue
                t = tables[j]
                _ck(L.mpqe_embed_l2norm_bwd(g.data_ptr() + 4 * i * D, N * D, _p(t), t.shape[0], D, _p(node_map),
                                            0 if node_map is None else node_map.shape[0],
                                            anchor_ids_t.data_ptr() + 8 * i * B, B, _p(gtabs[j]), _p(err),
                                            _stream()), 'mpqe_embed_l2norm_bwd')
            if gmode is not None:
                _ck(L.mpqe_var_rows_bwd(_p(g), mode_emb.shape[0], D, _p(var_ids), V, B, N, A, _p(gmode), _p(err),
                                        _stream()), 'mpqe_var_rows_bwd')
        return (gmode, None, None, None, None, None) + tuple(gtabs)


def assemble_x(mode_emb, node_map, anchor_ids_t, var_ids, slot_table, tables, err=None):
    return _AssembleX.apply(mode_emb, node_map, anchor_ids_t, var_ids, tuple(slot_table), err, *tables)


# --------------------------------------------------------------------------------------------- readouts
class _Readout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, kind, B, N, A):
        h = _f(h, 'embs')
        D = h.shape[1]
        if h.shape[0] != B * N:
            raise ValueError('embs has %d rows, expected batch_size*num_nodes = %d' % (h.shape[0], B * N))
        out = torch.empty((B, D), dtype=torch.float32, device=h.device)
        arg = torch.empty((B, D), dtype=torch.int32, device=h.device) if kind == 'max' else None
        with torch.cuda.device(h.device):
            _ck(lib().mpqe_readout_fwd(READOUT_IDS[kind], _p(h), B, N, A, D, _p(out), _p(arg), _stream()),
                'mpqe_readout_fwd')
        ctx.meta = (kind, B, N, A, D)
        ctx.save_for_backward(arg)
        return out

    @staticmethod
    def backward(ctx, g):
        kind, B, N, A, D = ctx.meta
        (arg,) = ctx.saved_tensors
        g = _f(g, 'grad')
        gh = torch.empty((B * N, D), dtype=torch.float32, device=g.device)
        with torch.cuda.device(g.device):
            _ck(lib().mpqe_readout_bwd(READOUT_IDS[kind], _p(g), _p(arg), B, N, A, D, _p(gh), _stream()),
                'mpqe_readout_bwd')
        return gh, None, None, None, None


def readout(kind, h, batch_size, num_nodes, num_anchors):
    """(a5) sum / max / mp(TM) over regular batches (row = b*N + n)."""
    return _Readout.apply(h, kind, int(batch_size), int(num_nodes), int(num_anchors))


class _Scatter(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, index, op, dim_size, err):
        src, index = _f(src, 'src'), _i(index, 'index')
        shape = src.shape
        src2 = src.reshape(shape[0], -1)
        n, D = src2.shape
        if index.dim() != 1 or index.shape[0] != n:
            raise ValueError('index must be 1-D with src.size(0) entries')
        L = lib()
        out = torch.empty((dim_size, D), dtype=torch.float32, device=src.device)
        arg = torch.empty((dim_size, D), dtype=torch.int64, device=src.device) if op == 'max' else None
        with torch.cuda.device(src.device):
            wb = L.mpqe_scatter_workspace_bytes(n, dim_size)
            ws = _ws(wb, src.device)
            _ck(L.mpqe_scatter_fwd(SCATTER_IDS[op], _p(src2), _p(index), n, D, dim_size, _p(out), _p(arg), _p(ws),
                                   wb, _p(err), _stream()), 'mpqe_scatter_fwd')
        ctx.meta = (op, n, D, dim_size, shape)
        ctx.save_for_backward(index, arg)
        out = out.reshape((dim_size,) + tuple(shape[1:]))
        if op == 'max':
            arg = arg.reshape(out.shape)
            ctx.mark_non_differentiable(arg)
            return out, arg
        return out

    @staticmethod
    def backward(ctx, g, *unused):
        op, n, D, dim_size, shape = ctx.meta
        index, arg = ctx.saved_tensors
        g = _f(g, 'grad').reshape(dim_size, D)
        L = lib()
        gs = torch.empty((n, D), dtype=torch.float32, device=g.device)
        with torch.cuda.device(g.device):
            wb = L.mpqe_scatter_workspace_bytes(n, dim_size)
            ws = _ws(wb, g.device)
            _ck(L.mpqe_scatter_bwd(SCATTER_IDS[op], _p(g), _p(index), _p(arg), n, D, dim_size, _p(gs), _p(ws), wb,
                                   _stream()), 'mpqe_scatter_bwd')
        return gs.reshape(shape), None, None, None, None


def _scatter(op, src, index, dim, dim_size):
    if dim != 0:
        raise NotImplementedError('mpqe_amd scatter ops reduce along dim 0 (all reference call sites do)')
    if dim_size is None:
        # the reference lets torch_scatter size the output from index.max() (one sync there too)
        dim_size = int(index.max().item()) + 1 if index.numel() else 0
    err = new_error_word(src.device)
    res = _Scatter.apply(src, index, op, int(dim_size), err)
    raise_on_flags(err)
    return res


def scatter_add(src, index, dim=0, out=None, dim_size=None, fill_value=0):
    """torch_scatter.scatter_add stand-in (reference call sites model.py:351, 381)."""
    return _scatter('add', src, index, dim, dim_size)


def scatter_mean(src, index, dim=0, out=None, dim_size=None, fill_value=0):
    return _scatter('mean', src, index, dim, dim_size)


def scatter_max(src, index, dim=0, out=None, dim_size=None, fill_value=None):
    """Returns (values, argmax) like torch_scatter (reference model.py:384)."""
    return _scatter('max', src, index, dim, dim_size)


# --------------------------------------------------------------------------------------------- (a9) LayerNorm + ReLU
class _LayerNormReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps, relu):
        x, gamma, beta = _f(x, 'x'), _f(gamma, 'gamma'), _f(beta, 'beta')
        rows, D = x.shape
        if gamma.shape != (D,) or beta.shape != (D,):
            raise ValueError('layer norm: gamma / beta must be [%d]' % D)
        y = torch.empty_like(x)
        stats = torch.empty((rows, 2), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _ck(lib().mpqe_layernorm_relu_fwd(_p(x), rows, D, _p(gamma), _p(beta), eps, int(relu), _p(y), _p(stats), _stream()),
                'mpqe_layernorm_relu_fwd')
        ctx.eps, ctx.relu = eps, bool(relu)
        ctx.save_for_backward(x, y, gamma, stats)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, y, gamma, stats = ctx.saved_tensors
        gy = _f(gy, 'grad_out')
        rows, D = x.shape
        gx = torch.empty_like(x)
        gg = torch.zeros(D, dtype=torch.float32, device=x.device)
        gb = torch.zeros(D, dtype=torch.float32, device=x.device)
        L = lib()
        with torch.cuda.device(x.device):
            wb = L.mpqe_layernorm_relu_bwd_workspace_bytes(rows, D)
            ws = _ws(wb, x.device)
            _ck(L.mpqe_layernorm_relu_bwd(_p(gy), _p(x), _p(y), rows, D, _p(gamma), _p(stats), ctx.eps, int(ctx.relu), _p(gx),
                                          _p(gg), _p(gb), _p(ws), wb, _stream()), 'mpqe_layernorm_relu_bwd')
        return gx, gg, gb, None, None


def layernorm_relu(x, gamma, beta, eps=1e-6, relu=True):
    """(a9) act(gamma * (x - mean) / (std + eps) + beta) per row, std UNBIASED (reference encoders.py:143-146), one kernel
    with the Encoder's ReLU (encoders.py:127-128)."""
    return _LayerNormReLU.apply(x, gamma, beta, float(eps), bool(relu))


# --------------------------------------------------------------------------------------------- score / loss
class _Cosine(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, t, q_row, eps):
        q, t = _f(q, 'query embeddings'), _f(t, 'target embeddings')
        q_row = None if q_row is None else _i(q_row, 'q_row')
        n, D = t.shape
        if q.shape[1] != D or (q_row is None and q.shape[0] != n):
            raise ValueError('cosine: shapes %s vs %s' % (tuple(q.shape), tuple(t.shape)))
        s = torch.empty((n,), dtype=torch.float32, device=q.device)
        with torch.cuda.device(q.device):
            _ck(lib().mpqe_cosine_fwd(_p(q), _p(q_row), _p(t), n, D, eps, _p(s), _stream()), 'mpqe_cosine_fwd')
        ctx.eps = eps
        ctx.save_for_backward(q, t, q_row)
        return s

    @staticmethod
    def backward(ctx, gs):
        q, t, q_row = ctx.saved_tensors
        gs = _f(gs, 'grad_scores')
        n, D = t.shape
        gq = (torch.zeros_like(q) if q_row is not None else torch.empty_like(q)) if ctx.needs_input_grad[0] else None
        gt = torch.empty_like(t) if ctx.needs_input_grad[1] else None
        with torch.cuda.device(q.device):
            _ck(lib().mpqe_cosine_bwd(_p(gs), _p(q), _p(q_row), _p(t), n, D, ctx.eps, _p(gq), _p(gt), _stream()),
                'mpqe_cosine_bwd')
        return gq, gt, None, None


def cosine(q, t, q_row=None, eps=1e-8):
    """(a6) F.cosine_similarity(q[q_row], t, dim=1)"""
    return _Cosine.apply(q, t, q_row, float(eps))


RANK_MAX_K = 128          # csrc/rank.hip: the per-query candidate lists live in LDS


def exclusion_csr(exclude, n_queries):
    """One list of table rows per query -> (offsets [Q+1], rows) int64 numpy, each list sorted and without repeats."""
    if len(exclude) != n_queries:
        raise ValueError('rank_entities: exclude must hold one list per query (%d for %d)' % (len(exclude), n_queries))
    lists = [np.unique(np.asarray(e, dtype=np.int64).reshape(-1)) for e in exclude]
    off = np.zeros(n_queries + 1, dtype=np.int64)
    if lists:
        off[1:] = np.cumsum([l.shape[0] for l in lists])
    rows = np.concatenate(lists) if lists else np.zeros(0, dtype=np.int64)
    return off, rows.astype(np.int64, copy=False)


RANK_SCORES = {'cosine': 0, 'dot': 1}


def rank_entities(q, table, target_rows=None, exclude=None, k=0, eps=1e-8, err=None, score='cosine'):
    """Every row of `table` ([N, D], raw rows) ranked against the query embeddings q [Q, D] by the model's score
    cos(q[i], table[r] / |table[r]|), or with score='dot' by q[i] . table[r]: mpqe_rank_entities_scored
    (include/mpqe_amd.h). Inference only: nothing here is differentiated. Everything is in table rows.
      target_rows  [Q] int64 or None
      exclude      None, one list of rows per query, or (offsets [Q+1], rows) int64 tensors (lists sorted ascending)
    -> (topk_rows [Q, k] int64, topk_scores [Q, k], rank [Q] int64 or None, target_scores [Q] or None); the first two
    are None for k = 0. Rows outside the table OR MPQE_FLAG_BAD_INDEX into `err` (ops.raise_on_flags)."""
    k = int(k)
    if k < 0 or k > RANK_MAX_K:
        raise ValueError('rank_entities: k must be in [0, %d], got %d' % (RANK_MAX_K, k))
    if score not in RANK_SCORES:
        raise ValueError('rank_entities: score must be one of %s, got %r' % (sorted(RANK_SCORES), score))
    if not torch.is_tensor(q) or not torch.is_tensor(table) or q.dim() != 2 or table.dim() != 2:
        raise ValueError('rank_entities: q and table must be 2-d tensors')
    if q.shape[1] != table.shape[1] or table.shape[0] < 1:
        raise ValueError('rank_entities: shapes %s vs %s' % (tuple(q.shape), tuple(table.shape)))
    Q, D = q.shape
    N = table.shape[0]
    if target_rows is not None and (not torch.is_tensor(target_rows) or tuple(target_rows.shape) != (Q,)):
        raise ValueError('rank_entities: target_rows must be a tensor of one row per query')
    if k == 0 and target_rows is None:
        raise ValueError('rank_entities: nothing to compute (k = 0 and no target_rows)')
    off = rows = None
    if exclude is not None:
        if isinstance(exclude, tuple) and len(exclude) == 2 and torch.is_tensor(exclude[0]):
            off, rows = exclude
            if tuple(off.shape) != (Q + 1,) or rows.dim() != 1:
                raise ValueError('rank_entities: exclude offsets must be [Q + 1], rows 1-d')
        else:
            off, rows = (torch.from_numpy(a) for a in exclusion_csr(exclude, Q))
    q, table = _f(q.detach(), 'query embeddings'), _f(table.detach(), 'embedding table')
    dev = q.device
    if target_rows is not None:
        target_rows = _i(target_rows, 'target_rows')
    E = 0
    if off is not None:
        E = int(rows.shape[0])
        off, rows = _i(off.to(dev), 'exclude offsets'), _i(rows.to(dev), 'exclude rows')
        if E == 0:
            off = rows = None
    topr = torch.empty((Q, k), dtype=torch.int64, device=dev) if k else None
    tops = torch.empty((Q, k), dtype=torch.float32, device=dev) if k else None
    rank = torch.empty((Q,), dtype=torch.int64, device=dev) if target_rows is not None else None
    tsc = torch.empty((Q,), dtype=torch.float32, device=dev) if target_rows is not None else None
    if Q == 0:
        return topr, tops, rank, tsc
    with torch.cuda.device(dev):
        need = lib().mpqe_rank_workspace_bytes(Q, N, D, k)
        if need == 0:
            raise ValueError('rank_entities: shape outside what the kernel covers')
        ws = _ws(need, dev)
        _ck(lib().mpqe_rank_entities_scored(_p(q), Q, _p(table), N, D, float(eps), RANK_SCORES[score], _p(target_rows),
                                            _p(off), _p(rows), E, k, _p(topr), _p(tops), _p(rank), _p(tsc), _p(ws), need,
                                            _p(err), _stream()), 'mpqe_rank_entities_scored')
    return topr, tops, rank, tsc


class RankMixedDescriptors(object):
    """The device block of mpqe_rank_mixed_desc_build (include/mpqe_amd.h): the candidate sets of a mixed ranking call.
      tables        one [rows_s, D] float32 tensor per set (raw rows, 16-byte aligned)
      scores        one of RANK_SCORES per set, or one name for all
      valid         None, or per set None / an int32 tensor of ceil(rows_s / 32) words (bit r clear: row r is no entity)
      set_of_group  one set index per group (a query names its group; in evaluation the group is the formula)
    It holds addresses and sizes only, so it is built once and kept (the tensors are held here, which keeps the
    addresses theirs); `addresses` lets the owner see that a tensor was replaced."""

    def __init__(self, tables, set_of_group, scores='cosine', valid=None):
        import ctypes
        tables = [_f(t.detach(), 'embedding table') for t in tables]
        if not tables or any(t.dim() != 2 or t.shape[1] != tables[0].shape[1] or t.shape[0] < 1 for t in tables):
            raise ValueError('rank_entities_mixed: every set a table [rows >= 1, D] with one D')
        S = len(tables)
        scores = [scores] * S if isinstance(scores, str) else list(scores)
        if len(scores) != S or any(s not in RANK_SCORES for s in scores):
            raise ValueError('rank_entities_mixed: one score of %s per set' % sorted(RANK_SCORES))
        valid = [None] * S if valid is None else list(valid)
        if len(valid) != S:
            raise ValueError('rank_entities_mixed: valid must hold one entry per set')
        for s, v in enumerate(valid):
            if v is None:
                continue
            valid[s] = v = _need(v, torch.int32, 'valid words')
            if v.dim() != 1 or v.shape[0] < (tables[s].shape[0] + 31) // 32:
                raise ValueError('rank_entities_mixed: valid words of set %d: ceil(rows / 32) int32 words' % s)
        sog = np.ascontiguousarray(set_of_group, dtype=np.int32).reshape(-1)
        G = int(sog.shape[0])
        self.tables, self.valid, self.scores = tables, valid, scores
        self.num_sets, self.num_groups, self.dim = S, G, int(tables[0].shape[1])
        self.rows = [int(t.shape[0]) for t in tables]
        self.max_rows, self.total_rows = max(self.rows), sum(self.rows)
        self.set_of_group = sog
        dev = tables[0].device
        L = lib()
        self.nbytes = L.mpqe_rank_mixed_desc_bytes(S, G)
        if self.nbytes == 0:
            raise ValueError('rank_entities_mixed: %d sets / %d groups outside [1, 256] / [1, 2^20]' % (S, G))
        self.buffer = torch.empty(self.nbytes + 256, dtype=torch.uint8, device=dev)
        self.ptr = _capi._align256(self.buffer.data_ptr())
        tab_arr = (ctypes.c_void_p * S)(*[_p(t) for t in tables])
        val_arr = (ctypes.c_void_p * S)(*[_p(v) for v in valid])
        rows_arr = (ctypes.c_int64 * S)(*self.rows)
        kind_arr = (ctypes.c_int32 * S)(*[RANK_SCORES[s] for s in scores])
        with torch.cuda.device(dev):
            _ck(L.mpqe_rank_mixed_desc_build(tab_arr, rows_arr, kind_arr, val_arr, S, sog.ctypes.data, G, self.ptr,
                                             self.nbytes, _stream()), 'mpqe_rank_mixed_desc_build')
        self.addresses = tuple(t.data_ptr() for t in tables)


def rank_entities_mixed(q, desc, group_of, target_rows=None, exclude_bits=None, k=0, eps=1e-8, err=None):
    """Q query embeddings ranked in ONE call, query i against candidate set desc.set_of_group[group_of[i]]
    (mpqe_rank_entities_mixed, include/mpqe_amd.h): bit for bit rank_entities over the queries of one set.
      group_of      [Q] int64 on the device
      target_rows   [Q] int64 rows of the query's own set, or None
      exclude_bits  None or [Q, W] int32 words: bit r of row i set = row r is not eligible for query i
    -> (topk_rows [Q, k], topk_scores [Q, k], rank [Q] or None, target_scores [Q] or None) as rank_entities. A group or a
    target row out of range ORs MPQE_FLAG_BAD_INDEX into `err`. Inference only."""
    k = int(k)
    if k < 0 or k > RANK_MAX_K:
        raise ValueError('rank_entities_mixed: k must be in [0, %d], got %d' % (RANK_MAX_K, k))
    if not torch.is_tensor(q) or q.dim() != 2 or q.shape[1] != desc.dim:
        raise ValueError('rank_entities_mixed: q must be [Q, %d]' % desc.dim)
    q = _f(q.detach(), 'query embeddings')
    Q, D = q.shape
    group_of = _i(group_of, 'group_of')
    if tuple(group_of.shape) != (Q,):
        raise ValueError('rank_entities_mixed: group_of must hold one group per query')
    if target_rows is not None:
        target_rows = _i(target_rows, 'target_rows')
        if tuple(target_rows.shape) != (Q,):
            raise ValueError('rank_entities_mixed: target_rows must hold one row per query')
    if k == 0 and target_rows is None:
        raise ValueError('rank_entities_mixed: nothing to compute (k = 0 and no target_rows)')
    W = 0
    if exclude_bits is not None:
        exclude_bits = _need(exclude_bits, torch.int32, 'exclude_bits')
        if exclude_bits.dim() != 2 or exclude_bits.shape[0] != Q or exclude_bits.shape[1] < 1:
            raise ValueError('rank_entities_mixed: exclude_bits must be [Q, W >= 1] int32 words')
        W = int(exclude_bits.shape[1])
    dev = q.device
    topr = torch.empty((Q, k), dtype=torch.int64, device=dev) if k else None
    tops = torch.empty((Q, k), dtype=torch.float32, device=dev) if k else None
    rank = torch.empty((Q,), dtype=torch.int64, device=dev) if target_rows is not None else None
    tsc = torch.empty((Q,), dtype=torch.float32, device=dev) if target_rows is not None else None
    if Q == 0:
        return topr, tops, rank, tsc
    with torch.cuda.device(dev):
        need = lib().mpqe_rank_mixed_workspace_bytes(Q, desc.num_sets, desc.max_rows, desc.total_rows, D, k)
        if need == 0:
            raise ValueError('rank_entities_mixed: shape outside what the kernel covers')
        buf = torch.empty(need + 256, dtype=torch.uint8, device=dev)
        ws = _capi._align256(buf.data_ptr())
        _ck(lib().mpqe_rank_entities_mixed(_p(q), Q, D, float(eps), desc.ptr, desc.nbytes, desc.num_sets, desc.num_groups,
                                           desc.max_rows, desc.total_rows, _p(group_of), _p(target_rows),
                                           _p(exclude_bits), W, k, _p(topr), _p(tops), _p(rank), _p(tsc), ws, need,
                                           _p(err), _stream()), 'mpqe_rank_entities_mixed')
    return topr, tops, rank, tsc


class _Hinge(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos, neg, margin):
        pos, neg = _f(pos, 'pos scores'), _f(neg, 'neg scores')
        if pos.shape != neg.shape or pos.dim() != 1 or pos.shape[0] == 0:
            raise ValueError('hinge: pos/neg must be equal non-empty vectors')
        # (0-dim from the start: a reshape here would make the result a VIEW created inside a Function, and the reference's
        # `loss += w * margin_loss(...)`, train_helpers.py:103-110, writes the first loss in place -- autograd refuses that)
        loss = torch.empty((), dtype=torch.float32, device=pos.device)
        with torch.cuda.device(pos.device):
            _ck(lib().mpqe_hinge_fwd(_p(pos), _p(neg), pos.shape[0], margin, _p(loss), _stream()), 'mpqe_hinge_fwd')
        ctx.margin = margin
        ctx.save_for_backward(pos, neg)
        return loss

    @staticmethod
    def backward(ctx, gl):
        pos, neg = ctx.saved_tensors
        gl = _f(gl.reshape(1), 'grad_loss')
        gp, gn = torch.empty_like(pos), torch.empty_like(neg)
        with torch.cuda.device(pos.device):
            _ck(lib().mpqe_hinge_bwd(_p(pos), _p(neg), pos.shape[0], ctx.margin, _p(gl), _p(gp), _p(gn), _stream()),
                'mpqe_hinge_bwd')
        return gp, gn, None


class _L2Norms(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *params):
        import ctypes
        ps = [_f(p, 'parameter') for p in params]
        out = torch.zeros((), dtype=torch.float32, device=ps[0].device)
        with torch.cuda.device(ps[0].device):
            for i in range(0, len(ps), 4):
                chunk = ps[i:i + 4]
                arr = (ctypes.c_void_p * len(chunk))(*[_p(p) for p in chunk])
                n = (ctypes.c_int64 * len(chunk))(*[p.numel() for p in chunk])
                _ck(lib().mpqe_l2_norms(arr, n, len(chunk), None, _p(out), None, _stream()), 'mpqe_l2_norms')
        ctx.save_for_backward(*ps)
        return out

    @staticmethod
    def backward(ctx, gl):
        import ctypes
        ps = ctx.saved_tensors
        gl = _f(gl.reshape(1), 'grad_out')
        grads = [torch.zeros_like(p) for p in ps]
        with torch.cuda.device(ps[0].device):
            for i in range(0, len(ps), 4):
                chunk, gch = ps[i:i + 4], grads[i:i + 4]
                arr = (ctypes.c_void_p * len(chunk))(*[_p(p) for p in chunk])
                garr = (ctypes.c_void_p * len(chunk))(*[_p(g) for g in gch])
                n = (ctypes.c_int64 * len(chunk))(*[p.numel() for p in chunk])
                _ck(lib().mpqe_l2_norms(arr, n, len(chunk), _p(gl), None, garr, _stream()), 'mpqe_l2_norms')
        return tuple(grads)


def l2_norms(params):
    """(a7) sum_i ||p_i||_2 over parameter tensors (unsquared: reference model.py:486-490), fixed order of every sum."""
    return _L2Norms.apply(*[p for p in params])


def hinge(pos, neg, margin=1.0):
    """(a7) mean(clamp(margin - (pos - neg), min=0))"""
    return _Hinge.apply(pos, neg, float(margin))


# --------------------------------------------------------------------------------------------- GQE baseline
class _BranchAgg(torch.autograd.Function):
    @staticmethod
    def forward(ctx, kind, *xs):
        if kind not in ('mean', 'min') or len(xs) not in (2, 3):
            raise ValueError('branch_agg: mean / min over two or three branches')
        xs = [_f(x, 'branch') for x in xs]
        if any(x.shape != xs[0].shape for x in xs):
            raise ValueError('branch_agg: branches of different shapes')
        out = torch.empty_like(xs[0])
        x2 = xs[2] if len(xs) == 3 else None
        with torch.cuda.device(out.device):
            _ck(lib().mpqe_branch_agg_fwd(_p(xs[0]), _p(xs[1]), _p(x2), out.numel(), int(kind == 'min'), _p(out), _stream()),
                'mpqe_branch_agg_fwd')
        ctx.kind = kind
        ctx.save_for_backward(*xs)
        return out

    @staticmethod
    def backward(ctx, g):
        xs = ctx.saved_tensors
        g = _f(g, 'grad')
        gs = [torch.empty_like(x) if ctx.needs_input_grad[1 + k] else None for k, x in enumerate(xs)]
        x2 = xs[2] if len(xs) == 3 else None
        g2 = gs[2] if len(xs) == 3 else None
        with torch.cuda.device(g.device):
            _ck(lib().mpqe_branch_agg_bwd(_p(xs[0]), _p(xs[1]), _p(x2), g.numel(), int(ctx.kind == 'min'), _p(g), _p(gs[0]),
                                          _p(gs[1]), _p(g2), _stream()), 'mpqe_branch_agg_bwd')
        return (None,) + tuple(gs)


def branch_agg(xs, kind):
    """mean / min over two or three equally shaped tensors, element by element (reference decoders.py:293-298: torch.stack +
    agg_func(dim=0)); a minimum's gradient goes to the first branch that holds it."""
    return _BranchAgg.apply(kind, *xs)


GQE_PROG_INTS = 32
GQE_MAX_DIM = 256


GQE_OPS = {'matrix': 0, 'translate': 1, 'scale': 2}
GQE_SCORES = {'cosine': 0, 'dot': 1}


def gqe_programme(form, branches, e_table, agg='mean', pre=-1, post=-1, tail=(), op='matrix', score='cosine'):
    """The int32 programme of mpqe_gqe_fwd / bwd (include/mpqe_amd.h). branches: [(table index, [(matrix index, transposed)])],
    tail: [(matrix index, transposed)] after the intersection; form 0 = chain, 1 = intersection. op: what a branch / tail
    site does with its parameter -- 'matrix' [D, D], 'translate' / 'scale' a [D] vector (`transposed` then means nothing);
    score: 'cosine' | 'dot'."""
    if op not in GQE_OPS or score not in GQE_SCORES:
        raise ValueError('gqe_programme: op %r / score %r' % (op, score))
    prog = np.full(GQE_PROG_INTS, -1, dtype=np.int32)
    prog[0], prog[1], prog[2], prog[3], prog[4], prog[5], prog[6], prog[7] = (form, len(branches), int(agg == 'min'), pre, post,
                                                                             len(tail), e_table, GQE_OPS[op])
    prog[27] = GQE_SCORES[score]
    for b, (table, steps) in enumerate(branches):
        prog[8 + 5 * b], prog[9 + 5 * b] = table, len(steps)
        for s, (m, t) in enumerate(steps):
            prog[10 + 5 * b + s] = 2 * m + int(bool(t))
    for s, (m, t) in enumerate(tail):
        prog[24 + s] = 2 * m + int(bool(t))
    return prog


def gqe_supported(dim):
    return dim % 16 == 0 and 16 <= dim <= GQE_MAX_DIM


def _gqe_check_params(prog, params, D, what):
    """Every parameter a programme names has the shape its site reads: [D] at a branch / tail site under a vector operator,
    [D, D] everywhere else (the kernel cannot see a shape: a [D] vector read as a matrix would be read past its end)."""
    vec = int(prog[7]) != 0
    sites = [(int(prog[10 + 5 * b + s]) >> 1, vec) for b in range(int(prog[1])) for s in range(int(prog[9 + 5 * b]))]
    sites += [(int(prog[24 + s]) >> 1, vec) for s in range(int(prog[5]))]
    sites += [(int(prog[k]), False) for k in (3, 4) if int(prog[k]) >= 0]
    for m, is_vec in sites:
        # (an index outside `params` is the entry point's to refuse)
        if 0 <= m < len(params) and tuple(params[m].shape) != ((D,) if is_vec else (D, D)):
            raise ValueError('%s: parameter %d of the programme must be %s' % (what, m, '[D]' if is_vec else '[D, D]'))


class _GqeScores(torch.autograd.Function):
    """One mpqe_gqe_fwd per forward, one mpqe_gqe_bwd per backward; the differentiable inputs are the entity tables and the
    matrices the programme names (`params` = tables, then matrices)."""

    @staticmethod
    def forward(ctx, spec, num_tables, *params):
        import ctypes
        tables = [_f(t, 'embedding table') for t in params[:num_tables]]
        mats = [_f(m, 'matrix') for m in params[num_tables:]]
        D = tables[0].shape[1]
        if any(t.dim() != 2 or t.shape[1] != D for t in tables) or any(tuple(m.shape) not in ((D, D), (D,)) for m in mats):
            raise ValueError('gqe_scores: every table [rows, D] and every parameter [D, D] or [D] with one D')
        prog, node_map, p_ids, e_ids, qrow, neg_off, n, err, eps = spec
        _gqe_check_params(prog, mats, D, 'gqe_scores')
        p_ids, e_ids = _i(p_ids, 'p_ids'), _i(e_ids, 'e_ids')
        node_map = None if node_map is None else _i(node_map, 'node_map')
        qrow = None if qrow is None else _i(qrow, 'qrow')
        neg_off = None if neg_off is None else _i(neg_off, 'neg_off')
        prog = np.ascontiguousarray(prog, dtype=np.int32)
        dev = tables[0].device
        p_rows = p_ids.shape[1]
        save = any(ctx.needs_input_grad[2:])
        L = lib()
        tab_arr = (ctypes.c_void_p * len(tables))(*[_p(t) for t in tables])
        rows_arr = (ctypes.c_int64 * len(tables))(*[t.shape[0] for t in tables])
        mat_arr = (ctypes.c_void_p * max(len(mats), 1))(*[_p(m) for m in mats])
        scores = torch.empty((n,), dtype=torch.float32, device=dev)
        ws, wb = None, 0
        with torch.cuda.device(dev):
            if save:
                wb = L.mpqe_gqe_workspace_bytes(prog.ctypes.data, p_rows, n, D)
                if wb == 0:
                    raise ValueError('gqe_scores: shape outside what the kernel covers')
                ws = _ws(wb + 256, dev)
            wp = None if ws is None else _capi._align256(ws.data_ptr())
            args = (prog.ctypes.data, tab_arr, rows_arr, len(tables), _p(node_map), 0 if node_map is None else node_map.shape[0],
                    mat_arr, len(mats), D, _p(p_ids), p_rows, _p(e_ids), e_ids.shape[0], _p(qrow), _p(neg_off), n, eps)
            _ck(L.mpqe_gqe_fwd(*(args + (int(save), _p(scores), wp, wb, _p(err), _stream()))), 'mpqe_gqe_fwd')
        ctx.call = (args, wp, wb, err, num_tables, (prog, tab_arr, rows_arr, mat_arr, ws, p_ids, e_ids, qrow, neg_off, node_map))
        ctx.save_for_backward(*(tables + mats))
        return scores

    @staticmethod
    def backward(ctx, gs):
        import ctypes
        args, wp, wb, err, num_tables, _keep = ctx.call
        params = ctx.saved_tensors
        gs = _f(gs, 'grad_scores')
        grads = [torch.zeros_like(p) if ctx.needs_input_grad[2 + k] else None for k, p in enumerate(params)]
        gt = (ctypes.c_void_p * num_tables)(*[_p(g) for g in grads[:num_tables]])
        gm = (ctypes.c_void_p * max(len(params) - num_tables, 1))(*[_p(g) for g in grads[num_tables:]])
        with torch.cuda.device(gs.device):
            _ck(lib().mpqe_gqe_bwd(*(args + (_p(gs), gt, gm, wp, wb, _p(err), _stream()))), 'mpqe_gqe_bwd')
        return (None, None) + tuple(grads)


def gqe_scores(prog, tables, mats, node_map, p_ids, e_ids, qrow, neg_off, n, err=None, eps=1e-8):
    """The GQE scores of one formula batch in one launch (mpqe_gqe_fwd, include/mpqe_amd.h), differentiable w.r.t. the
    entity tables and the matrices. p_ids [branches, p_rows], e_ids [e_rows], qrow [n] (chain form) / neg_off [B + 1]
    (intersection form with negatives) int64 on the device."""
    spec = (prog, node_map, p_ids, e_ids, qrow, neg_off, int(n), err, float(eps))
    return _GqeScores.apply(spec, len(tables), *(list(tables) + list(mats)))


def gqe_embed(prog, tables, mats, node_map, p_ids, p_rows, err=None):
    """The rows a GQE programme scores, [p_rows, D] float32 on the tables' device (mpqe_gqe_embed, include/mpqe_amd.h):
    the P side of gqe_scores alone -- lookup, normalisation, the products, the intersection -- with the forward's
    arithmetic. p_ids [branches, p_rows] int64 on the device, or None with one branch: row r of that branch's table is P
    row r (no ids, no node_map). Inference only: the inputs are detached, nothing here is differentiated."""
    import ctypes
    tables = [_f(t.detach(), 'embedding table') for t in tables]
    mats = [_f(m.detach(), 'matrix') for m in mats]
    D = tables[0].shape[1]
    if any(t.dim() != 2 or t.shape[1] != D for t in tables) or any(tuple(m.shape) not in ((D, D), (D,)) for m in mats):
        raise ValueError('gqe_embed: every table [rows, D] and every parameter [D, D] or [D] with one D')
    _gqe_check_params(prog, mats, D, 'gqe_embed')
    p_rows = int(p_rows)
    if p_ids is not None:
        p_ids = _i(p_ids, 'p_ids')
        if p_ids.dim() != 2 or p_ids.shape[1] != p_rows:
            raise ValueError('gqe_embed: p_ids must be [branches, p_rows]')
    node_map = None if node_map is None or p_ids is None else _i(node_map, 'node_map')
    prog = np.ascontiguousarray(prog, dtype=np.int32)
    dev = tables[0].device
    tab_arr = (ctypes.c_void_p * len(tables))(*[_p(t) for t in tables])
    rows_arr = (ctypes.c_int64 * len(tables))(*[t.shape[0] for t in tables])
    mat_arr = (ctypes.c_void_p * max(len(mats), 1))(*[_p(m) for m in mats])
    out = torch.empty((p_rows, D), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _ck(lib().mpqe_gqe_embed(prog.ctypes.data, tab_arr, rows_arr, len(tables), _p(node_map),
                                 0 if node_map is None else node_map.shape[0], mat_arr, len(mats), D, _p(p_ids), p_rows,
                                 _p(out), _p(err), _stream()), 'mpqe_gqe_embed')
    return out


class GqeMixedDescriptors(object):
    """The device block of mpqe_gqe_mixed_desc_build (include/mpqe_amd.h) for F programmes of one query type over one list
    of tables and one list of parameters: what a formula alone decides -- its tables, the parameter and transposition of
    every site. It depends on the programmes and on the ADDRESSES of the tables and parameters only, so it is built once
    and kept (the tensors are held here, which keeps the addresses theirs)."""

    def __init__(self, progs, tables, mats):
        import ctypes
        progs = np.ascontiguousarray(progs, dtype=np.int32)
        if progs.ndim != 2 or progs.shape[0] < 1 or progs.shape[1] != GQE_PROG_INTS:
            raise ValueError('gqe_scores_mixed: programmes [F >= 1, %d]' % GQE_PROG_INTS)
        tables = [_f(t.detach(), 'embedding table') for t in tables]
        mats = [_f(m.detach(), 'matrix') for m in mats]
        D = tables[0].shape[1]
        if any(t.dim() != 2 or t.shape[1] != D for t in tables) or any(tuple(m.shape) not in ((D, D), (D,)) for m in mats):
            raise ValueError('gqe_scores_mixed: every table [rows, D] and every parameter [D, D] or [D] with one D')
        for prog in progs:
            _gqe_check_params(prog, mats, D, 'gqe_scores_mixed')
        self.progs, self.tables, self.mats, self.dim = progs, tables, mats, int(D)
        self.num_formulas = int(progs.shape[0])
        dev = tables[0].device
        L = lib()
        self.nbytes = L.mpqe_gqe_mixed_desc_bytes(self.num_formulas)
        if self.nbytes == 0:
            raise ValueError('gqe_scores_mixed: more formulas than the kernel covers')
        self.buffer = torch.empty(self.nbytes + 256, dtype=torch.uint8, device=dev)
        self.ptr = _capi._align256(self.buffer.data_ptr())
        tab_arr = (ctypes.c_void_p * len(tables))(*[_p(t) for t in tables])
        rows_arr = (ctypes.c_int64 * len(tables))(*[t.shape[0] for t in tables])
        mat_arr = (ctypes.c_void_p * max(len(mats), 1))(*[_p(m) for m in mats])
        with torch.cuda.device(dev):
            _ck(L.mpqe_gqe_mixed_desc_build(progs.ctypes.data, self.num_formulas, tab_arr, rows_arr, len(tables), mat_arr,
                                            len(mats), D, self.ptr, self.nbytes, _stream()), 'mpqe_gqe_mixed_desc_build')
            # the index block of the mixed backward (mpqe_gqe_mixed_index_build): the table and parameter INDEX of every
            # slot and site; it depends on the programmes alone
            self.index_nbytes = L.mpqe_gqe_mixed_index_bytes(self.num_formulas)
            self.index_buffer = torch.empty(self.index_nbytes + 256, dtype=torch.uint8, device=dev)
            self.index_ptr = _capi._align256(self.index_buffer.data_ptr())
            _ck(L.mpqe_gqe_mixed_index_build(progs.ctypes.data, self.num_formulas, len(tables), len(mats), D, self.index_ptr,
                                             self.index_nbytes, _stream()), 'mpqe_gqe_mixed_index_build')
        self.addresses = tuple(t.data_ptr() for t in tables + mats)


def gqe_scores_mixed(desc, node_map, formula_of, p_ids, e_ids, qrow, neg_off, n, err=None, eps=1e-8):
    """The GQE scores of queries of DIFFERENT formulas of one query type in one launch (mpqe_gqe_fwd_mixed,
    include/mpqe_amd.h): gqe_scores' operands over the concatenation, formula_of [B] int64 on the device naming every
    query's programme in `desc` (a GqeMixedDescriptors, kept by the caller). -> fp32 [n], bit for bit what gqe_scores
    gives run by run. Inference only: nothing here is differentiated."""
    formula_of, p_ids, e_ids = _i(formula_of, 'formula_of'), _i(p_ids, 'p_ids'), _i(e_ids, 'e_ids')
    node_map = None if node_map is None else _i(node_map, 'node_map')
    qrow = None if qrow is None else _i(qrow, 'qrow')
    neg_off = None if neg_off is None else _i(neg_off, 'neg_off')
    n, B = int(n), int(formula_of.shape[0])
    if formula_of.dim() != 1 or p_ids.dim() != 2 or e_ids.dim() != 1:
        raise ValueError('gqe_scores_mixed: formula_of [B], p_ids [branches, p_rows], e_ids [e_rows]')
    dev = desc.tables[0].device
    scores = torch.empty((n,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _ck(lib().mpqe_gqe_fwd_mixed(desc.progs.ctypes.data, desc.num_formulas, desc.ptr, desc.nbytes, _p(node_map),
                                     0 if node_map is None else node_map.shape[0], desc.dim, _p(formula_of), B, _p(p_ids),
                                     int(p_ids.shape[1]), _p(e_ids), int(e_ids.shape[0]), _p(qrow), _p(neg_off), n,
                                     float(eps), _p(scores), _p(err), _stream()), 'mpqe_gqe_fwd_mixed')
    return scores


def gqe_embed_mixed(desc, node_map, formula_of, p_ids, err=None):
    """The rows gqe_scores_mixed would score, [B, D] float32, for queries of DIFFERENT formulas of one intersection type
    in one launch (mpqe_gqe_embed_mixed, include/mpqe_amd.h): bit for bit gqe_embed run by run. p_ids [branches, B]."""
    formula_of, p_ids = _i(formula_of, 'formula_of'), _i(p_ids, 'p_ids')
    node_map = None if node_map is None else _i(node_map, 'node_map')
    B = int(formula_of.shape[0])
    if formula_of.dim() != 1 or p_ids.dim() != 2 or p_ids.shape[1] != B:
        raise ValueError('gqe_embed_mixed: formula_of [B], p_ids [branches, B]')
    dev = desc.tables[0].device
    out = torch.empty((B, desc.dim), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _ck(lib().mpqe_gqe_embed_mixed(desc.progs.ctypes.data, desc.num_formulas, desc.ptr, desc.nbytes, _p(node_map),
                                       0 if node_map is None else node_map.shape[0], desc.dim, _p(formula_of), B, _p(p_ids),
                                       _p(out), _p(err), _stream()), 'mpqe_gqe_embed_mixed')
    return out


class _GqeScoresMixed(torch.autograd.Function):
    """One mpqe_gqe_fwd_mixed_save (mpqe_gqe_fwd_mixed when nothing needs a gradient) per forward, one mpqe_gqe_bwd_mixed per
    backward; the differentiable inputs are the descriptor's WHOLE table and parameter lists (`params` = tables, then
    parameters)."""

    @staticmethod
    def forward(ctx, spec, *params):
        desc, node_map, formula_of, p_ids, e_ids, qrow, neg_off, n, err, eps = spec
        T, M = len(desc.tables), len(desc.mats)
        if len(params) != T + M or tuple(_f(p, 'parameter').data_ptr() for p in params) != desc.addresses:
            raise ValueError('gqe_scores_mixed_grad: the tables and parameters are not the ones the descriptor block was '
                             'built on (their addresses differ): build a new GqeMixedDescriptors')
        B = int(formula_of.shape[0])
        dev = desc.tables[0].device
        save = any(ctx.needs_input_grad[1:])
        L = lib()
        scores = torch.empty((n,), dtype=torch.float32, device=dev)
        window = (_p(node_map), 0 if node_map is None else node_map.shape[0], desc.dim, _p(formula_of), B, _p(p_ids),
                  int(p_ids.shape[1]), _p(e_ids), int(e_ids.shape[0]), _p(qrow), _p(neg_off), n, eps)
        head = (desc.progs.ctypes.data, desc.num_formulas, desc.ptr, desc.nbytes)
        ws, wp, wb = None, None, 0
        with torch.cuda.device(dev):
            if save and B > 0:
                wb = L.mpqe_gqe_mixed_train_workspace_bytes(desc.progs.ctypes.data, desc.num_formulas, T, M,
                                                            int(p_ids.shape[1]), n, desc.dim)
                if wb == 0:
                    raise ValueError('gqe_scores_mixed_grad: shape outside what the kernel covers')
                ws = _ws(wb + 256, dev)
                wp = _capi._align256(ws.data_ptr())
                _ck(L.mpqe_gqe_fwd_mixed_save(*(head + (T, M) + window + (_p(scores), wp, wb, _p(err), _stream()))),
                    'mpqe_gqe_fwd_mixed_save')
            else:
                _ck(L.mpqe_gqe_fwd_mixed(*(head + window + (_p(scores), _p(err), _stream()))), 'mpqe_gqe_fwd_mixed')
        ctx.call = (desc, head, window, wp, wb, err, (ws, node_map, formula_of, p_ids, e_ids, qrow, neg_off))
        ctx.shapes = [tuple(p.shape) for p in params]
        return scores

    @staticmethod
    def backward(ctx, gs):
        import ctypes
        desc, head, window, wp, wb, err, _keep = ctx.call
        T, M = len(desc.tables), len(desc.mats)
        gs = _f(gs.contiguous(), 'grad_scores')
        dev = gs.device
        want = ctx.needs_input_grad[1:]
        # one zero-filled allocation for every wanted gradient, handed out as views (16-byte aligned: every size is a
        # multiple of D >= 16 floats)
        sizes = [int(np.prod(sh)) if w else 0 for sh, w in zip(ctx.shapes, want)]
        flat = torch.zeros(sum(sizes), dtype=torch.float32, device=dev)
        grads, at = [], 0
        for sh, w, k in zip(ctx.shapes, want, sizes):
            grads.append(flat[at:at + k].view(sh) if w else None)
            at += k
        if wp is not None:
            gt = (ctypes.c_void_p * T)(*[_p(g) for g in grads[:T]])
            gm = (ctypes.c_void_p * max(M, 1))(*[_p(g) for g in grads[T:]])
            with torch.cuda.device(dev):
                _ck(lib().mpqe_gqe_bwd_mixed(*(head + (desc.index_ptr, desc.index_nbytes, T, M) + window +
                                               (_p(gs), gt, gm, wp, wb, _p(err), _stream()))), 'mpqe_gqe_bwd_mixed')
        return (None,) + tuple(grads)


def gqe_scores_mixed_grad(desc, tables, mats, node_map, formula_of, p_ids, e_ids, qrow, neg_off, n, err=None, eps=1e-8):
    """gqe_scores_mixed, differentiable w.r.t. the descriptor's WHOLE table and parameter lists (`tables`, `mats`: the
    tensors `desc` was built on -- their data_ptr()s are checked, ValueError otherwise): mpqe_gqe_fwd_mixed_save when any
    of them needs a gradient (mpqe_gqe_fwd_mixed otherwise) and one mpqe_gqe_bwd_mixed in the backward
    (include/mpqe_amd.h). The scores are gqe_scores_mixed's bits. All gradients of a call are views of ONE zero-filled
    allocation; a parameter no query of the window names gets zeros, not None."""
    formula_of, p_ids, e_ids = _i(formula_of, 'formula_of'), _i(p_ids, 'p_ids'), _i(e_ids, 'e_ids')
    node_map = None if node_map is None else _i(node_map, 'node_map')
    qrow = None if qrow is None else _i(qrow, 'qrow')
    neg_off = None if neg_off is None else _i(neg_off, 'neg_off')
    if formula_of.dim() != 1 or p_ids.dim() != 2 or e_ids.dim() != 1:
        raise ValueError('gqe_scores_mixed_grad: formula_of [B], p_ids [branches, p_rows], e_ids [e_rows]')
    spec = (desc, node_map, formula_of, p_ids, e_ids, qrow, neg_off, int(n), err, float(eps))
    return _GqeScoresMixed.apply(spec, *(list(tables) + list(mats)))


# --------------------------------------------------------------------------------------------- R-GCN, mixed formulas
RGCN_MIX_MAX_PASSES = _capi.RGCN_MIX_MAX_PASSES


def rgcn_mixed_supported(dim, passes, readout):
    """The shapes mpqe_rgcn_fwd_mixed covers (include/mpqe_amd.h)."""
    return dim % 4 == 0 and 1 <= passes <= RGCN_MIX_MAX_PASSES and readout in READOUT_IDS


class RgcnMixedDescriptors(object):
    """The device block of mpqe_rgcn_mixed_desc_build (include/mpqe_amd.h) for F formulas of one query type over one list of
    entity tables: what a formula alone decides -- the relation of every template edge, the table of every anchor slot, the
    mode-embedding row of every variable slot, the target mode's table. recs [F, RGCN_MIX_REC_INTS] int32. It depends on the
    records and on the ADDRESSES of the tables only, so it is built once and kept (the tensors are held here, which keeps
    the addresses theirs); `ptrs` are those addresses, for a keeper that wants to know whether a tensor has moved."""

    def __init__(self, query_type, recs, tables, mode_emb_rows):
        import ctypes
        recs = np.ascontiguousarray(recs, dtype=np.int32)
        if recs.ndim != 2 or recs.shape[0] < 1 or recs.shape[1] != _capi.RGCN_MIX_REC_INTS:
            raise ValueError('rgcn_scores_mixed: records [F >= 1, %d]' % _capi.RGCN_MIX_REC_INTS)
        tables = [_f(t.detach(), 'embedding table') for t in tables]
        D = tables[0].shape[1]
        if any(t.dim() != 2 or t.shape[1] != D for t in tables):
            raise ValueError('rgcn_scores_mixed: every table [rows, D] with one D')
        self.query_type, self.qid = query_type, QUERY_TYPE_IDS[query_type]
        self.recs, self.tables, self.dim = recs, tables, int(D)
        self.num_formulas = int(recs.shape[0])
        self.ptrs = tuple(_p(t) for t in tables)
        dev = tables[0].device
        L = lib()
        self.nbytes = L.mpqe_rgcn_mixed_desc_bytes(self.num_formulas)
        if self.nbytes == 0:
            raise ValueError('rgcn_scores_mixed: more formulas than the kernel covers')
        self.buffer = torch.empty(self.nbytes + 256, dtype=torch.uint8, device=dev)
        self.ptr = _capi._align256(self.buffer.data_ptr())
        tab_arr = (ctypes.c_void_p * len(tables))(*self.ptrs)
        rows_arr = (ctypes.c_int64 * len(tables))(*[t.shape[0] for t in tables])
        with torch.cuda.device(dev):
            _ck(L.mpqe_rgcn_mixed_desc_build(self.qid, recs.ctypes.data, self.num_formulas, tab_arr, rows_arr, len(tables),
                                             int(mode_emb_rows), self.ptr, self.nbytes, _stream()),
                'mpqe_rgcn_mixed_desc_build')
            # the index block of the mixed backward (mpqe_rgcn_mixed_index_build): the table INDEX of every slot, the
            # relations and the mode-embedding rows; it depends on the records alone
            self.mode_emb_rows = int(mode_emb_rows)
            self.index_nbytes = L.mpqe_rgcn_mixed_index_bytes(self.num_formulas)
            self.index_buffer = torch.empty(self.index_nbytes + 256, dtype=torch.uint8, device=dev)
            self.index_ptr = _capi._align256(self.index_buffer.data_ptr())
            _ck(L.mpqe_rgcn_mixed_index_build(self.qid, recs.ctypes.data, self.num_formulas, self.index_ptr,
                                              self.index_nbytes, _stream()), 'mpqe_rgcn_mixed_index_build')


_RGCN_MIX_WS = {}        # device -> the mixed launches' workspace, grown in place (every call runs on the current stream)


def _rgcn_mixed_ws(nbytes, device):
    ws = _RGCN_MIX_WS.get(device)
    if ws is None or ws.shape[0] < nbytes + 256:
        ws = _RGCN_MIX_WS[device] = torch.empty(max(int(nbytes), 256) + 256, dtype=torch.uint8, device=device)
    return _capi._align256(ws.data_ptr())


def _rgcn_mixed_head(desc, node_map, mode_emb, layers, readout, formula_of, anchors):
    """the operands mpqe_rgcn_embed_mixed and mpqe_rgcn_fwd_mixed share, checked -> (argument tuple, tensors to keep alive)"""
    import ctypes
    formula_of, anchors = _i(formula_of, 'formula_of'), _i(anchors, 'anchors')
    node_map = None if node_map is None else _i(node_map, 'node_map')
    mode_emb = _f(mode_emb.detach(), 'mode_embeddings.weight')
    Q, D, passes = int(formula_of.shape[0]), desc.dim, len(layers)
    if formula_of.dim() != 1 or anchors.dim() != 2 or anchors.shape[0] != Q:
        raise ValueError('rgcn_scores_mixed: formula_of [B] and anchors [B, A]')
    if mode_emb.dim() != 2 or mode_emb.shape[1] != D or not rgcn_mixed_supported(D, passes, readout):
        raise ValueError('rgcn_scores_mixed: a shape the mixed launch does not cover')
    mats = []
    for basis, root, bias in layers:
        basis, root = _f(basis.detach(), 'basis'), _f(root.detach(), 'root')
        bias = None if bias is None else _f(bias.detach(), 'bias')
        if basis.dim() != 3 or tuple(basis.shape[1:]) != (D, D) or tuple(root.shape) != (D, D) or \
                basis.shape[0] != layers[0][0].shape[0]:
            raise ValueError('rgcn_scores_mixed: basis [R, D, D] and root [D, D] with one R and the tables\' D')
        mats.append((basis, root, bias))
    arr = [(ctypes.c_void_p * passes)(*[_p(m[k]) for m in mats]) for k in range(3)]
    wb = lib().mpqe_rgcn_mixed_workspace_bytes(desc.qid, Q, D)
    head = (desc.qid, desc.num_formulas, desc.ptr, desc.nbytes, _p(node_map), 0 if node_map is None else node_map.shape[0],
            _p(mode_emb), arr[0], arr[1], arr[2], int(mats[0][0].shape[0]), passes, READOUT_IDS[readout], D, _p(formula_of),
            _p(anchors), Q)
    return head, wb, (formula_of, anchors, node_map, mode_emb, mats, arr)


def rgcn_embed_mixed(desc, node_map, mode_emb, layers, readout, formula_of, anchors, err=None):
    """The R-GCN query embeddings [B, D] of queries of DIFFERENT formulas of one query type in one launch
    (mpqe_rgcn_embed_mixed): rgcn_scores_mixed's encode launch alone."""
    with torch.no_grad():
        head, wb, keep = _rgcn_mixed_head(desc, node_map, mode_emb, layers, readout, formula_of, anchors)
        dev = desc.tables[0].device
        q_out = torch.empty((head[-1], desc.dim), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _ck(lib().mpqe_rgcn_embed_mixed(*head, _rgcn_mixed_ws(wb, dev), wb, _p(q_out), _p(err), _stream()),
                'mpqe_rgcn_embed_mixed')
    return q_out


def rgcn_scores_mixed(desc, node_map, mode_emb, layers, readout, formula_of, anchors, ids, qrow, err=None, eps=1e-8):
    """The R-GCN model's scores of queries of DIFFERENT formulas of one query type in two launches (mpqe_rgcn_fwd_mixed,
    include/mpqe_amd.h). desc: an RgcnMixedDescriptors, kept by the caller; layers: [(basis, root, bias or None)], entry p
    what pass p runs; formula_of [B] and anchors [B, A] int64 on the device; ids [n] / qrow [n] the pairs in forward()'s
    layout. -> fp32 [n], bit for bit what the module path gives run by run. Inference only, under no_grad."""
    with torch.no_grad():
        head, wb, keep = _rgcn_mixed_head(desc, node_map, mode_emb, layers, readout, formula_of, anchors)
        ids, qrow = _i(ids, 'ids'), _i(qrow, 'qrow')
        n = int(ids.shape[0])
        if ids.dim() != 1 or qrow.dim() != 1 or qrow.shape[0] != n:
            raise ValueError('rgcn_scores_mixed: ids [n] and qrow [n]')
        dev = desc.tables[0].device
        scores = torch.empty((n,), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _ck(lib().mpqe_rgcn_fwd_mixed(*head, _p(ids), _p(qrow), n, float(eps), _rgcn_mixed_ws(wb, dev), wb, _p(scores),
                                          _p(err), _stream()), 'mpqe_rgcn_fwd_mixed')
    return scores


def rgcn_mixed_train_supported(dim, passes, readout, num_layers=1):
    """The shapes mpqe_rgcn_fwd_mixed_save / mpqe_rgcn_bwd_mixed cover (include/mpqe_amd.h)."""
    return (dim % 16 == 0 and 16 <= dim <= 256 and 1 <= passes <= RGCN_MIX_MAX_PASSES and readout in READOUT_IDS
            and 1 <= num_layers <= RGCN_MIX_MAX_PASSES)


class _RgcnMixedTrain(torch.autograd.Function):
    """One mpqe_rgcn_fwd_mixed_save per forward, one mpqe_rgcn_bwd_mixed per backward. The differentiable inputs are the
    descriptor's WHOLE table list, the mode embeddings and every distinct layer's basis / root / bias (`params` = tables,
    mode_emb, the bases, the roots, the biases that exist). embed: the query embeddings are returned and the backward goes
    through grad_q; otherwise the scores of ids [n] under neg_off."""

    @staticmethod
    def forward(ctx, spec, *params):
        import ctypes
        desc, node_map, layer_of_pass, has_bias, readout, formula_of, anchors, ids, neg_off, err, eps, embed = spec
        T, L, passes = len(desc.tables), len(has_bias), len(layer_of_pass)
        params = [_f(p, 'parameter') for p in params]
        tables, mode_emb = params[:T], params[T]
        basis, root = params[T + 1:T + 1 + L], params[T + 1 + L:T + 1 + 2 * L]
        biases, at = [], T + 1 + 2 * L
        for hb in has_bias:
            biases.append(params[at] if hb else None)
            at += 1 if hb else 0
        if tuple(t.data_ptr() for t in tables) != desc.ptrs:
            raise ValueError('rgcn_scores_mixed_grad: the tables are not the ones the descriptor block was built on (their '
                             'addresses differ): build a new RgcnMixedDescriptors')
        D, R = desc.dim, int(basis[0].shape[0])
        Q = int(formula_of.shape[0])
        n = 0 if embed else int(ids.shape[0])
        if mode_emb.dim() != 2 or mode_emb.shape[1] != D or mode_emb.shape[0] < desc.mode_emb_rows or \
                not rgcn_mixed_train_supported(D, passes, readout, L):
            raise ValueError('rgcn_scores_mixed_grad: a shape the mixed training launches do not cover')
        for b, r, bi in zip(basis, root, biases):
            if tuple(b.shape) != (R, D, D) or tuple(r.shape) != (D, D) or (bi is not None and tuple(bi.shape) != (D,)):
                raise ValueError('rgcn_scores_mixed_grad: basis [R, D, D], root [D, D] and bias [D] with one R and the tables\' D')
        dev = tables[0].device
        arr = [(ctypes.c_void_p * passes)(*[_p(seq[l]) for l in layer_of_pass]) for seq in (basis, root, biases)]
        head = (desc.qid, desc.num_formulas, desc.ptr, desc.nbytes)
        mid = (_p(node_map), 0 if node_map is None else node_map.shape[0], _p(mode_emb), arr[0], arr[1], arr[2], R, passes,
               READOUT_IDS[readout], D, _p(formula_of), _p(anchors), Q, _p(ids), _p(neg_off), n, eps, T,
               int(mode_emb.shape[0]), L)
        out = torch.empty((Q, D) if embed else (n,), dtype=torch.float32, device=dev)
        ws, wp, wb = None, None, 0
        if Q > 0:
            with torch.cuda.device(dev):
                wb = lib().mpqe_rgcn_mixed_train_workspace_bytes(desc.qid, Q, n, D, passes, R, T, int(mode_emb.shape[0]), L)
                if wb == 0:
                    raise ValueError('rgcn_scores_mixed_grad: shape outside what the kernels cover')
                ws = _ws(wb + 256, dev)
                wp = _capi._align256(ws.data_ptr())
                _ck(lib().mpqe_rgcn_fwd_mixed_save(*(head + mid + (wp, wb, None if embed else _p(out),
                                                                  _p(out) if embed else None, _p(err), _stream()))),
                    'mpqe_rgcn_fwd_mixed_save')
        ctx.call = (desc, head, mid, wp, wb, err, embed, list(layer_of_pass), has_bias,
                    (ws, node_map, formula_of, anchors, ids, neg_off, arr, params))
        ctx.shapes = [tuple(p.shape) for p in params]
        return out

    @staticmethod
    def backward(ctx, g):
        import ctypes
        desc, head, mid, wp, wb, err, embed, layer_of_pass, has_bias, _keep = ctx.call
        T, L = len(desc.tables), len(has_bias)
        g = _f(g.contiguous(), 'grad')
        dev = g.device
        want = ctx.needs_input_grad[1:]
        # one zero-filled allocation for every wanted gradient, handed out as views (16-byte aligned: every size is a
        # multiple of D >= 16 floats)
        sizes = [int(np.prod(sh)) if w else 0 for sh, w in zip(ctx.shapes, want)]
        flat = torch.zeros(sum(sizes), dtype=torch.float32, device=dev)
        grads, at = [], 0
        for sh, w, k in zip(ctx.shapes, want, sizes):
            grads.append(flat[at:at + k].view(sh) if w else None)
            at += k
        if wp is not None:
            gbias, at = [], T + 1 + 2 * L
            for hb in has_bias:
                gbias.append(grads[at] if hb else None)
                at += 1 if hb else 0
            gt = (ctypes.c_void_p * T)(*[_p(x) for x in grads[:T]])
            per = [(ctypes.c_void_p * L)(*[_p(x) for x in seq])
                   for seq in (grads[T + 1:T + 1 + L], grads[T + 1 + L:T + 1 + 2 * L], gbias)]
            lop = (ctypes.c_int * len(layer_of_pass))(*layer_of_pass)
            with torch.cuda.device(dev):
                _ck(lib().mpqe_rgcn_bwd_mixed(*(head + (desc.index_ptr, desc.index_nbytes) + mid + (
                    lop, None if embed else _p(g), _p(g) if embed else None, gt, _p(grads[T]), per[0], per[1], per[2], wp, wb,
                    _p(err), _stream()))), 'mpqe_rgcn_bwd_mixed')
        return (None,) + tuple(grads)


def _rgcn_mixed_train(desc, tables, mode_emb, layers, layer_of_pass, node_map, readout, formula_of, anchors, ids, neg_off, err,
                      eps, embed):
    formula_of, anchors = _i(formula_of, 'formula_of'), _i(anchors, 'anchors')
    node_map = None if node_map is None else _i(node_map, 'node_map')
    if formula_of.dim() != 1 or anchors.dim() != 2 or anchors.shape[0] != formula_of.shape[0]:
        raise ValueError('rgcn_scores_mixed_grad: formula_of [B] and anchors [B, A]')
    if not embed:
        ids, neg_off = _i(ids, 'ids'), _i(neg_off, 'neg_off')
        if ids.dim() != 1 or neg_off.dim() != 1 or neg_off.shape[0] != formula_of.shape[0] + 1 or \
                ids.shape[0] < formula_of.shape[0]:
            raise ValueError('rgcn_scores_mixed_grad: ids [B + total] and neg_off [B + 1]')
    has_bias = tuple(l[2] is not None for l in layers)
    params = list(tables) + [mode_emb] + [l[0] for l in layers] + [l[1] for l in layers] + \
        [l[2] for l in layers if l[2] is not None]
    spec = (desc, node_map, tuple(int(l) for l in layer_of_pass), has_bias, readout, formula_of, anchors, ids, neg_off, err,
            float(eps), embed)
    return _RgcnMixedTrain.apply(spec, *params)


def rgcn_scores_mixed_grad(desc, tables, mode_emb, layers, layer_of_pass, node_map, readout, formula_of, anchors, ids, neg_off,
                           err=None, eps=1e-8):
    """rgcn_scores_mixed with the pair layout fixed to forward()'s -- ids [B + total] = the B targets, then the negatives in
    CSR order under neg_off [B + 1] --, differentiable w.r.t. `tables` (the tensors `desc` was built on: their data_ptr()s
    are checked), `mode_emb` and every DISTINCT layer's (basis, root, bias or None) in `layers`; layer_of_pass[p]: the
    position in `layers` of what pass p runs. One mpqe_rgcn_fwd_mixed_save in the forward, one mpqe_rgcn_bwd_mixed in the
    backward (include/mpqe_amd.h); the scores are rgcn_scores_mixed's bits. All gradients of a call are views of ONE
    zero-filled allocation; a parameter no query of the window names gets zeros, not None."""
    return _rgcn_mixed_train(desc, tables, mode_emb, layers, layer_of_pass, node_map, readout, formula_of, anchors, ids,
                             neg_off, err, eps, False)


def rgcn_embed_mixed_grad(desc, tables, mode_emb, layers, layer_of_pass, node_map, readout, formula_of, anchors, err=None):
    """rgcn_embed_mixed, differentiable as rgcn_scores_mixed_grad is: the query embeddings [B, D], the backward through
    mpqe_rgcn_bwd_mixed's grad_q."""
    return _rgcn_mixed_train(desc, tables, mode_emb, layers, layer_of_pass, node_map, readout, formula_of, anchors, None, None,
                             err, 1e-8, True)


# --------------------------------------------------------------------------------------------- neighbourhood encoder
SAGE_MAX_DIM, SAGE_MAX_KEEP, SAGE_MAX_RELS = 256, _capi.SAGE_MAX_KEEP, _capi.SAGE_MAX_RELS


def sage_supported(dim_in, dim_out, num_rels=1, max_keep=1):
    """whether mpqe_sage_fwd covers the shape (include/mpqe_amd.h); what it does not is the caller's to route elsewhere"""
    return (dim_in % 16 == 0 and 16 <= dim_in <= SAGE_MAX_DIM and dim_out % 16 == 0 and 16 <= dim_out <= SAGE_MAX_DIM
            and 0 <= num_rels <= SAGE_MAX_RELS and 1 <= max_keep <= SAGE_MAX_KEEP)


class _SageEncode(torch.autograd.Function):
    """One mpqe_sage_fwd per forward, one mpqe_sage_bwd per backward; the differentiable inputs are the source matrices, the
    compress matrix and the normalisation's gamma / beta (`params` = tables, W[, gamma, beta])."""

    @staticmethod
    def forward(ctx, spec, num_tables, *params):
        import ctypes
        block_table, block_pad, neigh, counts, max_keep, self_rows, eps, err = spec
        tables = [_f(t, 'source matrix') for t in params[:num_tables]]
        W = _f(params[num_tables], 'compress matrix')
        ln = len(params) > num_tables + 1
        gamma = _f(params[num_tables + 1], 'gamma') if ln else None
        beta = _f(params[num_tables + 2], 'beta') if ln else None
        R = len(block_table) - 1
        din, dout = tables[0].shape[1], W.shape[0]
        if any(t.dim() != 2 or t.shape[1] != din for t in tables) or tuple(W.shape) != (dout, (R + 1) * din):
            raise ValueError('sage_encode: every source [rows, dim_in] and W [dim_out, (R + 1) dim_in]')
        self_rows = _i(self_rows, 'self_rows')
        B = self_rows.shape[0]
        if R:
            neigh = _i(neigh, 'neigh')
            counts = _need(counts, torch.int32, 'counts')
            if tuple(neigh.shape) != (R, B, max_keep) or tuple(counts.shape) != (R, B):
                raise ValueError('sage_encode: neigh [R, B, max_keep] and counts [R, B]')
        else:
            neigh = counts = None
        dev = W.device
        bt = np.ascontiguousarray(block_table, dtype=np.int32)
        bp = np.ascontiguousarray(block_pad, dtype=np.int64)
        tab_arr = (ctypes.c_void_p * len(tables))(*[_p(t) for t in tables])
        rows_arr = (ctypes.c_int64 * len(tables))(*[t.shape[0] for t in tables])
        save = any(ctx.needs_input_grad[2:])
        out = torch.empty((B, dout), dtype=torch.float32, device=dev)
        L = lib()
        ws, wp, wb = None, None, 0
        with torch.cuda.device(dev):
            if save:
                wb = L.mpqe_sage_workspace_bytes(B, R, din, dout, max_keep)
                if wb == 0:
                    raise ValueError('sage_encode: shape outside what the kernel covers (ops.sage_supported)')
                ws = _ws(wb + 256, dev)
                wp = _capi._align256(ws.data_ptr())
            args = (tab_arr, rows_arr, len(tables), bt.ctypes.data, bp.ctypes.data, R, _p(neigh), _p(counts), max_keep,
                    _p(self_rows), B, _p(W), din, dout, _p(gamma), _p(beta), eps)
            _ck(L.mpqe_sage_fwd(*(args + (int(save), _p(out), wp, wb, _p(err), _stream()))), 'mpqe_sage_fwd')
        ctx.call = (args, wp, wb, err, num_tables, (bt, bp, tab_arr, rows_arr, ws, neigh, counts, self_rows))
        ctx.save_for_backward(*(tables + [W] + ([gamma, beta] if ln else []) + [out]))
        return out

    @staticmethod
    def backward(ctx, g):
        import ctypes
        args, wp, wb, err, num_tables, _keep = ctx.call
        saved = ctx.saved_tensors
        params, out = saved[:-1], saved[-1]
        g = _f(g, 'grad_out')
        grads = [torch.zeros_like(p) if ctx.needs_input_grad[2 + k] else None for k, p in enumerate(params)]
        gt = (ctypes.c_void_p * num_tables)(*[_p(x) for x in grads[:num_tables]])
        gW = grads[num_tables]
        gg, gb = (grads[num_tables + 1], grads[num_tables + 2]) if len(params) > num_tables + 1 else (None, None)
        with torch.cuda.device(g.device):
            _ck(lib().mpqe_sage_bwd(*(args + (_p(out), _p(g), gt, _p(gW), _p(gg), _p(gb), wp, wb, _p(err), _stream()))),
                'mpqe_sage_bwd')
        return (None, None) + tuple(grads)


def sage_encode(tables, block_table, block_pad, neigh, counts, self_rows, W, gamma=None, beta=None, eps=1e-6, err=None):
    """Encoder.forward for a batch, given its sampled neighbours, in one launch (mpqe_sage_fwd, include/mpqe_amd.h) ->
    [B, dim_out]. tables: the source matrices [rows, dim_in]; block r of the compress matrix W [dim_out, (R + 1) dim_in] reads
    tables[block_table[r]] and its null row is block_pad[r]; neigh [R, B, max_keep] int64 / counts [R, B] int32 / self_rows
    [B] int64 on the device (rows; a negative self row is the null node). Differentiable w.r.t. the tables, W, gamma, beta."""
    if (gamma is None) != (beta is None):
        raise ValueError('sage_encode: gamma and beta come together')
    max_keep = int(neigh.shape[2]) if neigh is not None and len(block_table) > 1 else 1
    spec = (list(block_table), list(block_pad), neigh, counts, max_keep, self_rows, float(eps), err)
    params = list(tables) + [W] + ([gamma, beta] if gamma is not None else [])
    return _SageEncode.apply(spec, len(tables), *params)


# --------------------------------------------------------------------------------------------- evaluation metrics
def _eval_operand(t, dtype, what, lib_):
    """a contiguous tensor of `dtype`: on the GPU for the product library; wherever a stand-in `lib_` (the tests' host
    emulator of the kernels) can read it otherwise"""
    if lib_ is None:
        return _need(t, dtype, what)
    if not torch.is_tensor(t) or t.dtype != dtype:
        raise TypeError('mpqe_amd: %s must be a %s tensor' % (what, dtype))
    return t.contiguous()


def _eval_lib(device, lib_):
    """(library, stream) for a call on `device` (made current by the caller)"""
    return (lib(), _stream()) if lib_ is None else (lib_, None)


def eval_counts(scores, neg_offsets, B, lib=None, err=None):
    """counts [2, B] int64 on the scores' device (mpqe_eval_counts, include/mpqe_amd.h): per query the number of its
    negatives that score < / <= its target -- what scipy's percentileofscore takes (reference utils.py:25-32). scores
    [B + total] fp32 in forward()'s layout, neg_offsets [B + 1] int64. err: the caller's error word, read by the caller
    (a list whose offsets are out of order keeps garbage counts and sets FLAG_BAD_INDEX there); None: one of this call's,
    read before it returns (IndexError). lib: a bound C-ABI library to call instead of the product's, as on kg.KGIndex."""
    B = int(B)
    scores, neg_offsets = _eval_operand(scores, torch.float32, 'scores', lib), _eval_operand(neg_offsets, torch.int64,
                                                                                             'neg_offsets', lib)
    total = int(scores.shape[0]) - B
    if scores.dim() != 1 or neg_offsets.dim() != 1 or B < 0 or total < 0 or neg_offsets.shape[0] != B + 1:
        raise ValueError('eval_counts: scores [B + total] and neg_offsets [B + 1]')
    dev = scores.device
    own = err is None
    if own:
        err = new_error_word(dev)
    out = torch.empty((2, B), dtype=torch.int64, device=dev)
    if B:
        with (torch.cuda.device(dev) if lib is None else contextlib.nullcontext()):
            L, stream = _eval_lib(dev, lib)
            _capi.check(L, L.mpqe_eval_counts(_p(scores), _p(neg_offsets), B, total, _p(out), _p(err), stream),
                        'mpqe_eval_counts')
        if own:
            raise_on_flags(err)
    return out


def eval_percentiles(counts, neg_offsets):
    """float64 [B] on the device: scipy.stats.percentileofscore(kind='rank') from eval_counts' two counts -- (lt + le +
    (le > lt)) * 50.0 / n, NaN for n = 0. Every step is one correctly rounded IEEE operation (the integer sum is exact), so
    the values are evaluation.percentile_of_score's to the bit."""
    lt, le = counts[0], counts[1]
    n = (neg_offsets[1:] - neg_offsets[:-1]).to(torch.float64)
    return (lt + le + (le > lt).to(torch.int64)).to(torch.float64) * 50.0 / n


def eval_auc(pos, neg, lib=None):
    """The Python int U2 = sum over positives p of 2 |{neg < p}| + |{neg == p}| (mpqe_eval_auc, include/mpqe_amd.h), after
    np.nan_to_num's reading of the scores; ROC-AUC = U2 / (2 * len(pos) * len(neg)). pos, neg: fp32 vectors on the device.
    One 8-byte read. ValueError when either is empty, as sklearn's roc_auc_score has it."""
    pos, neg = _eval_operand(pos, torch.float32, 'pos', lib), _eval_operand(neg, torch.float32, 'neg', lib)
    if pos.dim() != 1 or neg.dim() != 1:
        raise ValueError('eval_auc: two score vectors')
    n_pos, n_neg = int(pos.shape[0]), int(neg.shape[0])
    if n_pos == 0 or n_neg == 0:
        raise ValueError('Only one class present in y_true. ROC AUC score is not defined in that case.')
    dev = pos.device
    out = torch.empty(1, dtype=torch.int64, device=dev)
    with (torch.cuda.device(dev) if lib is None else contextlib.nullcontext()):
        L, stream = _eval_lib(dev, lib)
        need = L.mpqe_eval_auc_workspace_bytes(n_pos, n_neg)
        if need == 0:
            raise ValueError('eval_auc: more scores than the kernel covers (2^31 a side)')
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        _capi.check(L, L.mpqe_eval_auc(_p(pos), n_pos, _p(neg), n_neg, _p(out), _p(ws), need, stream), 'mpqe_eval_auc')
    return int(out.item()) & (2 ** 64 - 1)


def auc_from_statistic(u2, n_pos, n_neg):
    """ROC-AUC from eval_auc's integer: one float64 division (what evaluation.roc_auc rounds to as well, n below 2^26)"""
    return u2 / (2 * n_pos * n_neg)


def eval_auc_segments(pos, neg, pos_off, neg_off, lib=None):
    """int64 [S] on the scores' device: eval_auc's integer U2 of every segment s -- pos[pos_off[s]:pos_off[s + 1]] against
    neg[neg_off[s]:neg_off[s + 1]] -- in one call with no host read (mpqe_eval_auc_segments, include/mpqe_amd.h); 0 where a
    side is empty. pos, neg: fp32 vectors, pos_off / neg_off: int64 [S + 1], all on the device. The caller copies the S
    integers once and divides (auc_from_statistic); a statistic is below 2^63 (2 n_pos n_neg < 2^63), so int64 holds it."""
    pos, neg = _eval_operand(pos, torch.float32, 'pos', lib), _eval_operand(neg, torch.float32, 'neg', lib)
    pos_off, neg_off = _eval_operand(pos_off, torch.int64, 'pos_off', lib), _eval_operand(neg_off, torch.int64, 'neg_off', lib)
    if pos.dim() != 1 or neg.dim() != 1 or pos_off.dim() != 1 or neg_off.dim() != 1 or pos_off.shape != neg_off.shape \
            or pos_off.shape[0] < 2:
        raise ValueError('eval_auc_segments: two score vectors and two offset vectors [S + 1], S >= 1')
    n_pos, n_neg, S = int(pos.shape[0]), int(neg.shape[0]), int(pos_off.shape[0]) - 1
    dev = pos.device
    out = torch.empty(S, dtype=torch.int64, device=dev)
    with (torch.cuda.device(dev) if lib is None else contextlib.nullcontext()):
        L, stream = _eval_lib(dev, lib)
        need = L.mpqe_eval_auc_segments_workspace_bytes(n_pos, n_neg, S)
        if need == 0:
            raise ValueError('eval_auc_segments: more scores or segments than the kernel covers (2^31)')
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        _capi.check(L, L.mpqe_eval_auc_segments(_p(pos), n_pos, _p(neg), n_neg, _p(pos_off), _p(neg_off), S, _p(out), _p(ws),
                                                need, stream), 'mpqe_eval_auc_segments')
    return out
