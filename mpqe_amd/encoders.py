"""Entity encoders with the reference's interface (mpqe/encoders.py).

DirectEncoder (reference encoders.py:11-45) is the depth-0 encoder every
BASELINE config uses: embedding lookup + L2 normalisation, here one fused HIP
kernel (gather through the global-id -> per-mode-row LUT, normalise, write).
"""
import random

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops


class DirectEncoder(nn.Module):
    """DirectEncoder(features, feature_modules[, node_maps])

    features         -- the reference's closure (nodes, mode) -> [B, D] embeddings. Only used when
                        `node_maps` is not given (then the lookup stays the caller's and just the
                        normalisation runs in the HIP kernel).
    feature_modules  -- {mode: nn.Embedding}; registered as "feat-<mode>" like the reference
                        (encoders.py:25-26) so state_dict keys match.
    node_maps        -- int64 LUT global entity id -> row of its mode's table, -1 for foreign ids
                        (what load_graph builds, data_utils.py:23-29). With it the whole
                        features(...) + normalise sequence is one kernel.
    """

    def __init__(self, features, feature_modules, node_maps=None):
        super(DirectEncoder, self).__init__()
        for name, module in feature_modules.items():
            self.add_module('feat-' + name, module)
        self.features = features
        self.feature_modules = feature_modules
        if node_maps is not None:
            self.register_buffer('node_maps', torch.as_tensor(node_maps, dtype=torch.long), persistent=False)
        else:
            self.node_maps = None
        self._err = None

    def table(self, mode):
        return self.feature_modules[mode].weight

    def error_word(self, device):
        if self._err is None or self._err.device != device:
            self._err = ops.new_error_word(device)
        return self._err

    def _ids(self, nodes, device):
        if not torch.is_tensor(nodes):
            nodes = torch.as_tensor(nodes, dtype=torch.long)
        return nodes.to(device=device, dtype=torch.long)

    def forward(self, nodes, mode, offset=None, **kwargs):
        """[D, B] unit-norm columns, like the reference (encoders.py:40-43)."""
        if offset is not None:
            raise NotImplementedError('EmbeddingBag offsets are never used by the R-GCN path')
        table = self.table(mode)
        if self.node_maps is not None:
            out = ops.embed_l2norm(table, self.node_maps, self._ids(nodes, table.device),
                                   self.error_word(table.device))
        else:
            emb = self.features(nodes, mode)
            rows = torch.arange(emb.shape[0], device=emb.device)
            out = ops.embed_l2norm(emb, None, rows, self.error_word(emb.device))
        return out.t()


class LayerNorm(nn.Module):
    """The Encoder's normalisation (reference encoders.py:132-146): per row, UNBIASED standard deviation, eps added to
    the standard deviation. Parameters `gamma` / `beta` as in the reference (state_dict keys `<mode>_ln.gamma|beta`).
    One HIP kernel (mpqe_layernorm_relu_fwd / bwd); `relu=True` folds the Encoder's activation into it."""

    def __init__(self, feature_dim, eps=1e-6):
        super(LayerNorm, self).__init__()
        self.gamma = nn.Parameter(torch.ones(feature_dim))
        self.beta = nn.Parameter(torch.zeros(feature_dim))
        self.eps = eps

    def forward(self, x, relu=False):
        lead = x.shape[:-1]
        y = ops.layernorm_relu(x.reshape(-1, x.shape[-1]), self.gamma, self.beta, self.eps, relu)
        return y.reshape(*lead, x.shape[-1])


class Encoder(nn.Module):
    """GraphSAGE-style entity encoder the reference inherits from GQE (encoders.py:47-129, `--depth >= 1`; SURVEY.md 8 a9,
    secondary row: unreachable from the R-GCN model in the reference itself). For a node of mode m:

        out = ReLU([LayerNorm](compress_m . [mean_r1 | ... | mean_rk | self]))        -> [out_dim, B]

    with mean_r = mean feature of the neighbours SAMPLED for relation r (python `random`, the reference's draws in the
    reference's order: aggregators.py). Constructor arguments, attribute names and state_dict keys (`<mode>_compress`,
    `<mode>_ln.gamma|beta`, `feat-<name>.*`) are the reference's; the data path is this package's:
      * ONE flat list of sampled neighbours per relation goes through the features closure and the scatter kernel
        (mean mode) -- no dense [B, U] mask matrix, no per-node python set arithmetic on the device side;
      * the concatenation is never materialised: compress_m is applied block by block (one mpqe_linear_fwd per relation
        block and one for the self block, accumulating), which is the same sum;
      * LayerNorm and the ReLU are one kernel (mpqe_layernorm_relu_fwd).
    `nodes` is a python list of entity ids (the GQE call protocol).

    With `index` (a kg.KGIndex over the graph's adjacency) the whole forward runs on the device: the draws are the index's
    (KGIndex.sample_neighbours, one launch for all relations of the mode; the library's stream, seeded per call by one
    random.getrandbits(64), so random.seed(...) still makes a run repeatable) and gather, means, product, LayerNorm and ReLU
    are ONE launch (ops.sage_encode, mpqe_sage_fwd). `nodes` may then also be an int64 tensor of entity ids on any device;
    a negative id is the null node. The null neighbour and the null node are the padding row of a table (its last row), not
    the reference's out-of-range lookup of node_maps[-1]. With a device `base_model` (depth >= 2) the sampled neighbours and
    the batch are first encoded by it -- one call per destination mode, with the DEFAULT keep_prob / max_keep, as the
    reference's lambdas do (utils.py:113-114) -- null slots as null nodes, nothing compacted, and the outer launch reads
    those matrices by position. `self_model`: the encoder of the node's own features where it is not base_model (the
    reference's enc3, utils.py:123); it is not registered as a submodule. The samples of the last call stay readable in
    `last_sample`. Shapes mpqe_sage_fwd does not cover (ops.sage_supported) keep the device draws and run on the per-op
    kernels of the host path (scatter mean, block-wise dense layer, LayerNorm + ReLU)."""

    def __init__(self, features, feature_dims, out_dims, relations, adj_lists, aggregator, base_model=None,
                 cuda=False, layer_norm=False, feature_modules={}, index=None, node_maps=None, self_model=None):
        super(Encoder, self).__init__()
        self.index, self.node_maps, self.feature_modules, self.last_sample = index, node_maps, feature_modules, None
        self._self_model = [self_model if self_model is not None else base_model]      # (a list: not a submodule)
        self._err = None
        self.features, self.feat_dims, self.out_dims = features, feature_dims, out_dims
        self.relations, self.adj_lists, self.aggregator = relations, adj_lists, aggregator
        self.cuda, self.layer_norm = cuda, layer_norm
        if self.aggregator is not None:
            self.aggregator.cuda = cuda
        if base_model is not None:
            self.base_model = base_model
        for name, module in feature_modules.items():
            self.add_module('feat-' + name, module)
        # per mode: the column blocks of its compress matrix -- one per outgoing relation (width = feature dim of the
        # relation's target mode), then the node's own features
        self.blocks, self.compress_dims, self.compress_params, self.lns = {}, {}, {}, {}
        for mode in relations:
            widths = [feature_dims[to_mode] for (to_mode, _) in relations[mode]] + [feature_dims[mode]]
            self.blocks[mode] = [(sum(widths[:k]), w) for k, w in enumerate(widths)]
            self.compress_dims[mode] = sum(widths)
        for mode in feature_dims:
            if layer_norm:
                self.lns[mode] = LayerNorm(out_dims[mode])
                self.add_module(mode + '_ln', self.lns[mode])
            w = nn.Parameter(torch.empty(out_dims[mode], self.compress_dims[mode]))
            nn.init.xavier_uniform_(w)
            self.compress_params[mode] = w
            self.register_parameter(mode + '_compress', w)

    def forward(self, nodes, mode, keep_prob=0.5, max_keep=10):
        if self.index is not None:
            return self.encode_rows(self.index.rows_of(mode, nodes), mode, keep_prob, max_keep).t()
        W = self.compress_params[mode]
        blocks = self.blocks[mode]
        feats = []
        for (to_mode, name), (off, width) in zip(self.relations[mode], blocks[:-1]):
            rel = (mode, name, to_mode)
            adj = self.adj_lists[rel]
            # the null neighbour -1 stands in for a padding node and for a node without edges of this relation
            neigh = [[-1] if (n == -1 or len(adj[n]) == 0) else adj[n] for n in nodes]
            feats.append(self.aggregator.forward(neigh, rel, keep_prob, max_keep).contiguous())    # [B, width]
        feats.append(self.features(nodes, mode).contiguous())
        # compress_m applied block by block on the library's own MFMA tiles (mpqe_linear_fwd, accumulating): the column
        # blocks of W are read in place, the concatenation of the reference (encoders.py:120) is never built
        out = ops.blocks_linear(feats, W, blocks)
        if self.layer_norm:
            out = self.lns[mode](out, relu=True)
        else:
            out = F.relu(out)
        return out.t()

    # ------------------------------------------------------------------ the device path (index given)
    def error_word(self, device):
        if self._err is None or self._err.device != device:
            self._err = ops.new_error_word(device)
        return self._err

    def _inner(self, requests):
        """requests: [(encoder, mode, rows)] -> (matrices, [(matrix index, first position)] per request, records). The
        requests of one (encoder, mode) share ONE call of that encoder, made with the default keep_prob / max_keep; every
        matrix ends in the encoding of one null node, its padding row."""
        groups, where = [], []
        for model, mode, rows in requests:
            for g, (m, md, parts) in enumerate(groups):
                if m is model and md == mode:
                    break
            else:
                g = len(groups)
                groups.append((model, mode, []))
            parts = groups[g][2]
            where.append((g, sum(int(p.shape[0]) for p in parts)))
            parts.append(rows.reshape(-1))
        mats, records = [], []
        for model, mode, parts in groups:
            rows = torch.cat(parts + [torch.full((1,), -1, dtype=torch.int64, device=parts[0].device)])
            mats.append(model.encode_rows(rows, mode))
            records.append({'encoder': 'base' if model is getattr(self, 'base_model', None) else 'self', 'mode': mode,
                            'rows': rows, 'sample': model.last_sample})
        return mats, where, records

    def encode_rows(self, rows, mode, keep_prob=0.5, max_keep=10):
        """forward() for table ROWS of `mode` (device int64; negative: the null node) -> [B, out_dim]"""
        index, W = self.index, self.compress_params[mode]
        dev = W.device
        rows = rows.to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
        B, max_keep = int(rows.shape[0]), int(max_keep)
        err = self.error_word(dev)
        rels = [(mode, name, to_mode) for to_mode, name in self.relations[mode]]
        R = len(rels)
        neigh = counts = None
        seed = random.getrandbits(64)
        if R:
            _, neigh, counts = index.sample_neighbours(mode, rows, keep_prob, max_keep, seed, relations=rels, err=err)
        base = getattr(self, 'base_model', None)
        sample = {'mode': mode, 'rows': rows, 'relations': rels, 'neigh': neigh, 'counts': counts, 'seed': seed,
                  'keep_prob': keep_prob, 'max_keep': max_keep, 'inner': None}
        if base is None:
            # depth 1: the sources are the embedding tables, one per mode met; the padding row is a table's last
            modes = []
            for m in [r[2] for r in rels] + [mode]:
                if m not in modes:
                    modes.append(m)
            tables = [self.feature_modules[m].weight for m in modes]
            block_table = [modes.index(r[2]) for r in rels] + [modes.index(mode)]
            block_pad = [int(tables[t].shape[0]) - 1 for t in block_table]
            src_neigh, self_rows = neigh, rows
        else:
            # depth >= 2: every sampled slot (a null slot as a null node) and the batch itself through the inner encoders
            self_model = self._self_model[0]
            requests = [(base, r[2], neigh[k]) for k, r in enumerate(rels)] + [(self_model, mode, rows)]
            tables, where, records = self._inner(requests)
            sample['inner'], sample['where'] = records, where
            block_table = [g for g, _ in where]
            block_pad = [int(tables[g].shape[0]) - 1 for g in block_table]
            slots = torch.arange(B * max_keep, dtype=torch.int64, device=dev).view(B, max_keep)
            src_neigh = torch.stack([slots + first for _, first in where[:-1]]) if R else None
            self_rows = torch.arange(B, dtype=torch.int64, device=dev) + where[-1][1]
        self.last_sample = sample
        ln = self.lns[mode] if self.layer_norm else None
        din, dout = int(tables[0].shape[1]), int(W.shape[0])
        if all(int(t.shape[1]) == din for t in tables) and ops.sage_supported(din, dout, R, max_keep) and W.shape[1] == (R + 1) * din:
            return ops.sage_encode(tables, block_table, block_pad, src_neigh, counts, self_rows, W,
                                   None if ln is None else ln.gamma, None if ln is None else ln.beta,
                                   1e-6 if ln is None else ln.eps, err)
        # a shape the fused kernel does not cover: the same samples through the per-op kernels of the host path
        feats = []
        for k in range(R):
            table, pad = tables[block_table[k]], block_pad[k]
            used = torch.arange(max_keep, device=dev)[None, :] < counts[k][:, None]
            picks = torch.where(used, src_neigh[k], torch.full_like(src_neigh[k], pad))
            used[:, 0] |= counts[k] == 0                     # the single null neighbour of a node without any
            seg = torch.arange(B, device=dev)[:, None].expand(B, max_keep)[used]
            feats.append(ops.scatter_mean(table[picks[used]].contiguous(), seg, dim=0, dim_size=B).contiguous())
        table, pad = tables[block_table[R]], block_pad[R]
        feats.append(table[torch.where(self_rows < 0, torch.full_like(self_rows, pad), self_rows)].contiguous())
        out = ops.blocks_linear(feats, W, self.blocks[mode])
        return ln(out, relu=True) if ln is not None else F.relu(out)
