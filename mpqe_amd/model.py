"""The R-GCN query encoder with the reference's module surface (mpqe/model.py:206-553):
same class names, constructor arguments, forward()/margin_loss() signatures, attributes
and state_dict keys -- every float computed by the gfx950 kernels behind include/mpqe_amd.h.
"""
import math
import random

import numpy as np
import torch
import torch.nn as nn

from . import _capi, ops
from .data_utils import RGCNQueryDataset
from .graph import reverse_relation
from .ops import scatter_add, scatter_max, scatter_mean  # noqa: F401  (re-exported like the reference)


def sample_negatives(graph, formula, queries, hard_negatives=False):
    """One negative per query by the reference's three rules (model.py:120-127 = 466-476), on python's `random` stream in
    the reference's order: shared by RGCNEncoderDecoder and QueryEncoderDecoder."""
    if "inter" not in formula.query_type and hard_negatives:
        raise Exception("Hard negative examples can only be used with "
                        "intersection queries")
    elif hard_negatives:
        return [random.choice(query.hard_neg_samples) for query in queries]
    elif formula.query_type == "1-chain":
        return [random.choice(graph.full_lists[formula.target_mode]) for _ in queries]
    return [random.choice(query.neg_samples) for query in queries]


class RGCNConv(nn.Module):
    """reference: RGCNConv, model.py:206-310 (a vendored PyG <= 1.4 layer).

        out_i = sum_{(j -> i, r)} x_j . basis[r]  +  x_i . root  +  bias

    'add' aggregation, no edge normalisation (the reference always passes edge_norm=None,
    model.py:436, 441). num_bases must be 0 as in the reference's only construction site
    (model.py:346); the basis-decomposition branch is not built.
    """

    def __init__(self, in_channels, out_channels, num_relations, num_bases, bias=True):
        super(RGCNConv, self).__init__()
        if num_bases != 0:
            raise NotImplementedError('basis decomposition (num_bases > 0) is never reached by the '
                                      'reference (model.py:346 hard-codes 0) and is not built')
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.num_relations = num_relations
        self.num_bases = num_bases
        self.basis = nn.Parameter(torch.Tensor(num_relations, in_channels, out_channels))
        self.att = None
        self.root = nn.Parameter(torch.Tensor(in_channels, out_channels))
        if bias:
            self.bias = nn.Parameter(torch.Tensor(out_channels))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        # reference model.py:258-267: every tensor ~ U(-b, b), b = 1/sqrt(num_relations*in_channels)
        bound = 1.0 / math.sqrt(self.num_relations * self.in_channels)
        for p in (self.basis, self.root, self.bias):
            if p is not None:
                p.data.uniform_(-bound, bound)

    def forward(self, x, edge_index, edge_type, edge_norm=None, relu=False):
        """x [N_total, in] -> [N_total, out]. `relu=True` fuses the F.relu the encoder applies
        after all but the last layer (model.py:437) into the kernel epilogue."""
        if edge_norm is not None:
            raise NotImplementedError('edge_norm is always None on the reference path (model.py:436, 441)')
        if x is None or x.dtype == torch.long:
            raise NotImplementedError('featureless (x=None / long x) RGCNConv is never used by the reference')
        graph = getattr(edge_index, '_mpqe_graph', None)
        if graph is None or (isinstance(graph, ops.GraphPlan) and
                             (graph.Nn != x.shape[0] or getattr(edge_index, '_mpqe_et', None) is not edge_type)):
            graph = ops.GraphPlan(edge_index, edge_type, x.shape[0], self.num_relations)
            edge_index._mpqe_graph = graph           # sorted once, reused by later layers / backward
            edge_index._mpqe_et = edge_type
        return ops.rgcn_layer(x, self.basis, self.root, self.bias, graph, relu)

    def __repr__(self):
        return '{}({}, {}, num_relations={})'.format(self.__class__.__name__, self.in_channels,
                                                     self.out_channels, self.num_relations)


class _EntityRanking(object):
    """Answering a query over ALL entities of the target mode, the part RGCNEncoderDecoder and QueryEncoderDecoder share:
    the row <-> id maps of a mode (cached in self.__dict__['_row_ids'] / ['_maps_np'], which __getstate__ drops), the id
    translation, the exclusion lists as CSR and the ops.rank_entities call. A model supplies the two operands."""

    def _mode_rows(self, mode, device):
        """(row -> global id [n] int64 on the device, rows below n that are no entity, the map on the host) of one mode, from
        graph.full_lists[mode] through enc.node_maps; built once per mode. n = 1 + the last row that is an entity: the
        tables carry a spare row at the end (data_utils.make_feature_modules), which is never ranked."""
        cache = self.__dict__.get('_row_ids')
        if cache is None:
            cache = self.__dict__['_row_ids'] = {}
        hit = cache.get(mode)
        if hit is not None and hit[0].device == device:
            return hit
        ids = np.asarray(list(self.graph.full_lists[mode]), dtype=np.int64)
        maps = self._maps_host()
        if ids.size == 0 or ids.min() < 0 or ids.max() >= maps.shape[0]:
            raise IndexError('mpqe_amd: full_lists[%r] is empty or holds ids outside node_maps' % (mode,))
        rows = maps[ids]
        if rows.min() < 0 or rows.max() >= self.enc.table(mode).shape[0]:
            raise IndexError('mpqe_amd: full_lists[%r] holds ids that are not of this mode' % (mode,))
        row_ids = np.full(int(rows.max()) + 1, -1, dtype=np.int64)
        row_ids[rows] = ids
        hit = (torch.from_numpy(row_ids).to(device), np.nonzero(row_ids < 0)[0].astype(np.int64), row_ids)
        cache[mode] = hit
        return hit

    def _maps_host(self):
        # (ONE host copy of node_maps, shared by the row maps of every mode and by the id translation of every call)
        m = self.__dict__.get('_maps_np')
        if m is None:
            m = self.__dict__['_maps_np'] = self.enc.node_maps.detach().cpu().numpy()
        return m

    def _rank_rows(self, formula, queries, target_nodes, exclude, k, operands):
        """Every entity of formula.target_mode ranked for each query: (ids [B, k] or None, scores, ranks [B] or None).
        operands(n) -> (q [B, D], candidates [n, D]) or (q, candidates, score): the two sides of ops.rank_entities over the
        mode's first n rows, and its score kind ('cosine' when left out)."""
        enc = self.enc
        if not (hasattr(enc, 'table') and getattr(enc, 'node_maps', None) is not None):
            raise NotImplementedError('answering a query needs the entity tables (DirectEncoder with node_maps)')
        device = self._device()
        B = len(queries)
        mode = formula.target_mode
        row_ids, holes, row_ids_host = self._mode_rows(mode, device)
        n = row_ids.shape[0]
        err = self._error_word(device)
        maps_host = self._maps_host()

        def rows_of(ids):
            # an id of another mode (node_maps gives it a row of ITS table), of no mode or outside node_maps becomes row n:
            # outside the ranked rows, so the kernel flags it and _check raises
            ids = np.asarray(ids, dtype=np.int64).reshape(-1)
            inside = (ids >= 0) & (ids < maps_host.shape[0])
            cand = np.where(inside, maps_host[np.where(inside, ids, 0)], -1)
            ok = (cand >= 0) & (cand < n)
            ok &= row_ids_host[np.where(ok, cand, 0)] == ids
            return np.where(ok, cand, n)

        target_rows = None
        if target_nodes is not None:
            t = target_nodes.detach().cpu().numpy() if torch.is_tensor(target_nodes) else target_nodes
            target_rows = torch.from_numpy(rows_of(t)).to(device)
            if target_rows.shape[0] != B:
                raise ValueError('one target per query')
        csr = None
        from .kg import KGAnswers
        if isinstance(exclude, KGAnswers):
            # exact answers from the device index (mpqe_amd/kg.py): the bitmaps OR the mode's holes, compacted on the device
            if exclude.mode != mode or exclude.n != n or len(exclude) != B:
                raise ValueError('exclude: KGAnswers of %d queries over %d rows of %r, ranking %d queries over %d rows of %r'
                                 % (len(exclude), exclude.n, exclude.mode, B, n, mode))
            csr = exclude.exclusion_csr()
        elif exclude is not None:
            if len(exclude) != B:
                raise ValueError('exclude must hold one id list per query')
            # one translation and one sort for the whole batch: keys (query, row), unique, then the segment bounds
            lens = np.fromiter((len(e) for e in exclude), dtype=np.int64, count=B)
            flat = np.fromiter((x for e in exclude for x in e), dtype=np.int64, count=int(lens.sum()))
            rows = np.concatenate([rows_of(flat), np.tile(holes, B)])
            owner = np.concatenate([np.repeat(np.arange(B, dtype=np.int64), lens),
                                    np.repeat(np.arange(B, dtype=np.int64), holes.size)])
            keys = np.unique(owner * (n + 1) + rows)
            off = np.searchsorted(keys, np.arange(B + 1, dtype=np.int64) * (n + 1)).astype(np.int64)
            csr = (torch.from_numpy(off), torch.from_numpy(keys % (n + 1)))
        elif holes.size:
            # rows of the table that are no entity: the same list for every query, kept on the device for the LAST batch size
            # seen per mode (one entry per mode: an evaluation loop's ragged last batch rebuilds it once, nothing accumulates)
            cache = self.__dict__['_row_ids']
            hit = cache.get(('holes', mode))
            if hit is None or hit[0] != B or hit[1][0].device != device:
                off = torch.arange(B + 1, dtype=torch.int64) * holes.size
                hit = cache[('holes', mode)] = (B, (off.to(device), torch.from_numpy(np.tile(holes, B)).to(device)))
            csr = hit[1]
        q, table, score = (tuple(operands(n)) + ('cosine',))[:3]
        topr, tops, rank, _ = ops.rank_entities(q, table, target_rows, csr, k, err=err, score=score)
        self._check()
        ids = None
        if topr is not None:
            ids = torch.where(topr >= 0, row_ids[topr.clamp(min=0)], topr)
        return ids, tops, rank

    # ------------------------------------------------------------------ ranking ids that are on the device already
    def rank_ids(self, formula, anchors, targets, exclude=None, k=0):
        """rank_targets / answer for ids that are on the device already (kg.QuerySet: evaluation.eval_rank_queries): anchors
        [B, A] and targets [B] int64; exclude a kg.KGAnswers of these queries (KGIndex.answers) or None. -> (ranks [B],
        top-k ids [B, k] or None, top-k scores), under no_grad: the per-formula route -- the model's own operands and ONE
        ops.rank_entities -- with the targets translated on the device (an id that is no entity of the target mode becomes
        the row past the ranked ones, so _check() raises). The by-runs fallback and the oracle of rank_ids_mixed."""
        from .kg import KGAnswers
        with torch.no_grad():
            device = self._device()
            mode = formula.target_mode
            row_ids, holes, _ = self._mode_rows(mode, device)
            n = row_ids.shape[0]
            anchors, targets, _, _ = _device_ids(anchors, targets, None, device, len(formula.anchor_modes))
            B = int(targets.shape[0])
            maps = self.enc.node_maps
            inside = (targets >= 0) & (targets < maps.shape[0])
            cand = torch.where(inside, maps[targets.clamp(0, maps.shape[0] - 1)], torch.full_like(targets, -1))
            ok = (cand >= 0) & (cand < n)
            ok &= row_ids[cand.clamp(0, n - 1)] == targets
            target_rows = torch.where(ok, cand, torch.full_like(cand, n))
            csr = None
            if isinstance(exclude, KGAnswers):
                if exclude.mode != mode or exclude.n != n or len(exclude) != B:
                    raise ValueError('exclude: KGAnswers of %d queries over %d rows of %r, ranking %d queries over %d rows of %r'
                                     % (len(exclude), exclude.n, exclude.mode, B, n, mode))
                csr = exclude.exclusion_csr()
            elif exclude is not None:
                raise TypeError('rank_ids: exclude is a kg.KGAnswers or None')
            elif holes.size:
                off = torch.arange(B + 1, dtype=torch.int64, device=device) * holes.size
                csr = (off, torch.from_numpy(holes).to(device).repeat(B))
            q, table, score = self._rank_operands_ids(formula, anchors, n)
            topr, tops, rank, _ = ops.rank_entities(q, table, target_rows, csr, k, err=self._error_word(device), score=score)
            self._check()
            ids = None if topr is None else torch.where(topr >= 0, row_ids[topr.clamp(min=0)], topr)
        return rank, ids, tops

    def _rank_mixed_sets(self, formulas, device):
        """The candidate sets of rank_ids_mixed for `formulas`: the distinct target modes, one ops.RankMixedDescriptors
        over the modes' tables (valid words from a mode's holes), and what translates ids on the device. Kept beside the
        row maps (self.__dict__['_row_ids'], reset where they are), keyed like _mixed_descriptors' entries: the identity of
        `formulas` and data_ptr() of every table the block points at."""
        cache = self.__dict__.get('_row_ids')
        if cache is None:
            cache = self.__dict__['_row_ids'] = {}
        modes = []
        for f in formulas:
            if f.target_mode not in modes:
                modes.append(f.target_mode)
        ptrs = tuple(self.enc.table(m).data_ptr() for m in modes)
        key = ('rank_mixed', id(formulas))
        hit = cache.get(key)
        if hit is not None and hit['formulas'] is formulas and hit['ptrs'] == ptrs and hit['device'] == device:
            return hit
        maps = [self._mode_rows(m, device) for m in modes]
        tables, valid = [], []
        for m, (row_ids, holes, row_ids_host) in zip(modes, maps):
            n = row_ids.shape[0]
            tables.append(self.enc.table(m).detach()[:n])
            words = None
            if holes.size:
                words = cache.get(('valid', m))
                if words is None or words.device != device:
                    bits = np.zeros((n + 31) // 32 * 32, dtype=bool)
                    bits[:n] = row_ids_host >= 0
                    words = np.packbits(bits.reshape(-1, 32), axis=1, bitorder='little').view('<u4').reshape(-1)
                    words = cache[('valid', m)] = torch.from_numpy(words.view(np.int32).copy()).to(device)
            valid.append(words)
        rows = np.asarray([t.shape[0] for t in tables], dtype=np.int64)
        base = np.zeros(len(modes), dtype=np.int64)
        base[1:] = np.cumsum(rows)[:-1]
        set_of_group = np.asarray([modes.index(f.target_mode) for f in formulas], dtype=np.int32)
        hit = {'formulas': formulas, 'ptrs': ptrs, 'device': device, 'modes': modes,
               'desc': ops.RankMixedDescriptors(tables, set_of_group, 'cosine', valid),
               'row_ids': torch.cat([m[0] for m in maps]), 'base': torch.from_numpy(base).to(device),
               'rows': torch.from_numpy(rows).to(device), 'set_of_group': torch.from_numpy(set_of_group.astype(np.int64)).to(device),
               'rows_host': [m[2] for m in maps], 'indexes': []}
        olds = [k for k in cache if isinstance(k, tuple) and k[0] == 'rank_mixed' and k != key]
        for old in olds[:max(0, len(olds) - (self.MIXED_KEPT - 1))]:         # (the oldest leave first)
            cache.pop(old)
        cache[key] = hit
        return hit

    def rank_ids_mixed(self, formulas, formula_of, anchors, targets, exclude=None, k=0):
        """rank_ids for queries of DIFFERENT formulas of one query type (kg.MixedQuerySet): `formulas` a sequence of Formula
        of that type (pass the SAME object every time), formula_of [B] int64 every query's position in it; exclude a
        kg.KGAnswersMixed of these queries with its bitmaps kept (KGIndex.answers_mixed) or None. -> (ranks, top-k ids,
        top-k scores) equal to rank_ids run by run, under no_grad. Where the model's mixed embedding covers the formulas
        (_embed_mixed) this is one embedding call and ONE ops.rank_entities_mixed over the distinct target modes: the
        answers' bitmaps are the exclusion words as they stand, targets and top-k rows are translated on the device.
        Otherwise the runs of equal formula are walked through rank_ids (rank_ids_by_runs)."""
        from .kg import KGAnswersMixed
        if not torch.is_tensor(formula_of) or formula_of.dtype != torch.long or formula_of.dim() != 1:
            raise TypeError('rank_ids_mixed: formula_of must be an int64 vector')
        if exclude is not None and not isinstance(exclude, KGAnswersMixed):
            raise TypeError('rank_ids_mixed: exclude is a kg.KGAnswersMixed or None')
        if exclude is not None and exclude.bits is None:
            raise ValueError('rank_ids_mixed: the answers were computed without their bitmaps (bits=False or chunked)')
        with torch.no_grad():
            if len(formulas) == 0 or len({f.query_type for f in formulas}) != 1:
                raise ValueError('rank_ids_mixed: formulas of one query type')
            device = self._device()
            anchors, targets, _, _ = _device_ids(anchors, targets, None, device, len(formulas[0].anchor_modes))
            B = int(targets.shape[0])
            if formula_of.shape[0] != B or (exclude is not None and len(exclude) != B):
                raise ValueError('rank_ids_mixed: formula_of [B], exclude of B queries')
            formula_of = formula_of.to(device).contiguous()
            q = self._embed_mixed(formulas, formula_of, anchors) if B and device.type == 'cuda' else None
            if q is None:
                return rank_ids_by_runs(self, formulas, formula_of.cpu().numpy(), anchors, targets, exclude, k)
            sets = self._rank_mixed_sets(formulas, device)
            if exclude is not None and not any(ix is exclude.index for ix in sets['indexes']):
                # once per `formulas` and index: the index numbers the rows of every target mode as the model does
                for m, host in zip(sets['modes'], sets['rows_host']):
                    if not np.array_equal(exclude.index.row_ids_host.get(m), host):
                        raise ValueError('rank_ids_mixed: the index\'s rows of mode %r are not the model\'s' % (m,))
                sets['indexes'].append(exclude.index)
            set_of = sets['set_of_group'][formula_of.clamp(0, len(formulas) - 1)]
            n, base = sets['rows'][set_of], sets['base'][set_of]
            maps = self.enc.node_maps
            inside = (targets >= 0) & (targets < maps.shape[0])
            cand = torch.where(inside, maps[targets.clamp(0, maps.shape[0] - 1)], torch.full_like(targets, -1))
            ok = (cand >= 0) & (cand < n)
            ok &= sets['row_ids'][base + torch.minimum(cand.clamp(min=0), n - 1)] == targets
            target_rows = torch.where(ok, cand, n)
            bits = None if exclude is None else exclude.bits.to(device)
            topr, tops, rank, _ = ops.rank_entities_mixed(q, sets['desc'], formula_of, target_rows, bits, k,
                                                          err=self._error_word(device))
            self._check()
            ids = None
            if topr is not None:
                ids = torch.where(topr >= 0, sets['row_ids'][base[:, None] + topr.clamp(min=0)], topr)
        return rank, ids, tops


class RGCNEncoderDecoder(nn.Module, _EntityRanking):
    """reference: RGCNEncoderDecoder, model.py:313-494."""

    def __init__(self, graph, enc, readout='mp', scatter_op='add', dropout=0, weight_decay=1e-3,
                 num_layers=3, shared_layers=True, adaptive=True):
        super(RGCNEncoderDecoder, self).__init__()
        self.enc = enc
        self.graph = graph
        self.emb_dim = graph.feature_dims[next(iter(graph.feature_dims))]
        self.mode_embeddings = nn.Embedding(len(graph.mode_weights), self.emb_dim)
        self.num_layers = num_layers
        self.adaptive = adaptive

        self.mode_ids = {mode: i for i, mode in enumerate(graph.mode_weights)}
        self.rel_ids = {}
        for r1 in graph.relations:
            for r2 in graph.relations[r1]:
                self.rel_ids[(r1, r2[1], r2[0])] = len(self.rel_ids)

        self.layers = nn.ModuleList()
        for i in range(num_layers):
            if len(self.layers) == 0 or not shared_layers:
                rgcn = RGCNConv(in_channels=self.emb_dim, out_channels=self.emb_dim,
                                num_relations=len(graph.rel_edges), num_bases=0)
            self.layers.append(rgcn)

        if scatter_op == 'add':
            scatter_fn = scatter_add
        elif scatter_op == 'max':
            scatter_fn = scatter_max
        elif scatter_op == 'mean':
            scatter_fn = scatter_mean
        else:
            raise ValueError(f'Unknown scatter op {scatter_op}')

        self.readout_str = readout
        if readout == 'sum':
            self.readout = self.sum_readout
        elif readout == 'max':
            self.readout = self.max_readout
        elif readout == 'mlp':
            self.readout = MLPReadout(self.emb_dim, self.emb_dim, scatter_fn)
        elif readout == 'targetmlp':
            self.readout = TargetMLPReadout(self.emb_dim, scatter_fn)
        elif readout == 'concat':
            self.readout = MLPReadout(self.emb_dim * num_layers, self.emb_dim, scatter_fn)
        elif readout == 'mp':
            self.readout = self.target_message_readout
        else:
            raise ValueError(f'Unknown readout function {readout}')

        self.dropout = nn.Dropout(dropout)      # built and never applied, as in the reference (model.py:377)
        self.weight_decay = weight_decay
        # the reference encodes the same query graphs twice per margin_loss (model.py:478-482);
        # the query embedding does not depend on the target, so it is computed once here and
        # scored twice. Set True for the reference's literal op sequence.
        self.encode_twice = False
        # one 4-byte D2H read per call to turn a bad id into IndexError (see ops.raise_on_flags)
        self.validate = True
        self._err = None
        # margin_loss / forward-without-autograd on the fused step (mpqe_amd/dropin.py): one library call per margin_loss for
        # the loss value, ONE fused step per backward pass for all of them. False: the per-op module path below (also taken
        # by foreign encoders, by encode_twice and by configurations the fused step does not cover).
        self.fused = True
        self._dropin_state = None
        from .optim import register_model
        register_model(self)            # (mpqe_amd.optim.Adam / SGD find the model of the parameters they are handed)

    # ------------------------------------------------------------------ readouts (model.py:380-398)
    def sum_readout(self, embs, batch_idx, batch_size=None, num_nodes=None, **kwargs):
        if batch_size is not None and num_nodes is not None and embs.shape[0] == batch_size * num_nodes:
            return ops.readout('sum', embs, batch_size, num_nodes, kwargs.get('num_anchors', 0))
        return scatter_add(embs, batch_idx, dim=0)

    def max_readout(self, embs, batch_idx, batch_size=None, num_nodes=None, **kwargs):
        if batch_size is not None and num_nodes is not None and embs.shape[0] == batch_size * num_nodes:
            return ops.readout('max', embs, batch_size, num_nodes, kwargs.get('num_anchors', 0))
        out, argmax = scatter_max(embs, batch_idx, dim=0)
        return out

    def target_message_readout(self, embs, batch_size, num_nodes, num_anchors, **kwargs):
        return ops.readout('mp', embs, batch_size, num_nodes, num_anchors)

    # ------------------------------------------------------------------ helpers
    def _device(self):
        return next(self.parameters()).device

    def _error_word(self, device):
        if self._err is None or self._err.device != device:
            self._err = ops.new_error_word(device)
        return self._err

    def _node_features(self, formula, anchor_ids, var_ids, device):
        """x [B*N, D]: anchors = normalised entity embeddings, variables = mode embeddings
        (model.py:418-422)."""
        enc = self.enc
        if hasattr(enc, 'table') and getattr(enc, 'node_maps', None) is not None:
            modes = list(formula.anchor_modes)
            uniq = []
            for m in modes:
                if m not in uniq:
                    uniq.append(m)
            ids_t = anchor_ids.to(device).t().contiguous()
            return ops.assemble_x(self.mode_embeddings.weight, enc.node_maps, ids_t, var_ids,
                                  [uniq.index(m) for m in modes], [enc.table(m) for m in uniq],
                                  self._error_word(device))
        # a foreign encoder: keep its call protocol (enc(ids, mode) -> [D, B])
        cols = [self.enc(anchor_ids[:, i], mode).t() for i, mode in enumerate(formula.anchor_modes)]
        var = self.mode_embeddings.weight[var_ids]
        B = anchor_ids.shape[0]
        x = torch.cat([c[:, None, :] for c in cols] + [var[None].expand(B, -1, -1)], dim=1)
        return x.reshape(-1, self.emb_dim)

    def encode(self, formula, queries, anchor_ids=None, var_ids=None, q_graphs=None):
        """Query embeddings [B, D] (everything in model.py:404-449 that precedes the scoring)."""
        if anchor_ids is None or var_ids is None or q_graphs is None:
            anchor_ids, var_ids, q_graphs = RGCNQueryDataset.get_query_graph(formula, queries, self.rel_ids,
                                                                             self.mode_ids)
        device = self._device()
        var_ids = var_ids.to(device)
        q_graphs = q_graphs.to(device)
        batch_size, num_anchors = anchor_ids.shape
        n_nodes = num_anchors + var_ids.shape[0]

        x = self._node_features(formula, anchor_ids, var_ids, device)
        q_graphs.x = x

        if self.adaptive:
            num_passes = RGCNQueryDataset.query_diameters[formula.query_type]
            if num_passes > len(self.layers):
                raise ValueError(f'RGCN is adaptive with {len(self.layers)}'
                                 f' layers, but query requires {num_passes}.')
        else:
            num_passes = self.num_layers

        h1 = x
        h_layers = []
        for i in range(num_passes - 1):
            h1 = self.layers[i](h1, q_graphs.edge_index, q_graphs.edge_type, relu=True)
            if self.readout_str == 'concat':
                h_layers.append(h1)
        h1 = self.layers[-1](h1, q_graphs.edge_index, q_graphs.edge_type)
        if self.readout_str == 'concat':
            h_layers.append(h1)
            h1 = torch.cat(h_layers, dim=1)

        return self.readout(embs=h1, batch_idx=q_graphs.batch, batch_size=batch_size, num_nodes=n_nodes,
                            num_anchors=num_anchors)

    def _target_embeds(self, nodes, mode, device):
        enc = self.enc
        if hasattr(enc, 'table') and getattr(enc, 'node_maps', None) is not None:
            ids = nodes if torch.is_tensor(nodes) else torch.as_tensor(nodes, dtype=torch.long)
            return ops.embed_l2norm(enc.table(mode), enc.node_maps, ids.to(device=device, dtype=torch.long),
                                    self._error_word(device))
        return self.enc(nodes, mode).t()

    def score(self, formula, out, target_nodes, neg_nodes=None, neg_lengths=None):
        """reference: model.py:451-462."""
        device = out.device
        scores = ops.cosine(out, self._target_embeds(target_nodes, formula.target_mode, device))
        if neg_nodes is not None:
            neg_embeds = self._target_embeds(neg_nodes, formula.target_mode, device)
            lengths = torch.as_tensor(neg_lengths, dtype=torch.long)
            q_row = torch.repeat_interleave(torch.arange(lengths.shape[0]), lengths).to(device)
            neg_scores = ops.cosine(out, neg_embeds, q_row=q_row)
            scores = torch.cat((scores, neg_scores), dim=0)
        return scores

    def _check(self):
        if self.validate:
            for err in (self._err, getattr(self.enc, '_err', None)):
                if err is not None:
                    ops.raise_on_flags(err)

    # ------------------------------------------------------------------ the fused step behind the entry points
    def __getstate__(self):
        # (copy.deepcopy / torch.save of the whole module: the fused step's bookkeeping -- device buffers, argument blocks,
        # the C++ pass object -- belongs to THIS object and is rebuilt by the copy at its first call)
        state = self.__dict__.copy()
        state['_dropin_state'] = None
        state['_dropin_checked'] = False
        state['_err'] = None
        state['_row_ids'] = None        # (the row -> id maps answer() caches on the device)
        state['_maps_np'] = None
        state['_mixed'] = None          # (score_ids_mixed's descriptor blocks: device addresses)
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)
        from .optim import register_model
        register_model(self)

    def _apply(self, fn, *args, **kwargs):
        # (.to() / .cuda() / .float(): the parameters move -- the fused step's addresses are taken again at the next call)
        out = super(RGCNEncoderDecoder, self)._apply(fn, *args, **kwargs)
        self.__dict__['_dropin_checked'] = False
        self.__dict__['_row_ids'] = None
        self.__dict__['_maps_np'] = None
        self.__dict__['_mixed'] = None
        return out

    def dropin(self):
        """The model's DropIn (mpqe_amd/dropin.py), or None when this model takes the module path."""
        if not self.fused or self.encode_twice:
            return None
        d = self._dropin_state
        if d is False:
            return None
        if d is not None and self.__dict__.get('_dropin_checked'):
            return d                # (nothing moved the parameters since the addresses were taken: _apply resets the flag;
                                    # FlatOptimizer, which re-homes them, refreshes the step's pointers itself)
        self.__dict__['_dropin_checked'] = True
        if d is not None and d.stale() and d.refresh():
            return d
        if d is None or d.stale():
            from .dropin import DropIn
            enc = self.enc
            try:
                if not (hasattr(enc, 'table') and getattr(enc, 'node_maps', None) is not None):
                    raise ValueError('foreign encoder')
                if self._device().type != 'cuda':
                    raise ValueError('not on the GPU')          # (the module path raises the package's usual error)
                d = DropIn(self)
            except (ValueError, NotImplementedError):
                d = False
            self.__dict__['_dropin_state'] = d
        return d or None

    def _fused_covers(self, d, formula, n_queries):
        # (concat reads one block per layer: the reference's own Linear fails on fewer passes; huge batches: the in-step
        # touch plan's limit -- both stay on the module path)
        if d.step.learned and self.readout_str == 'concat' and d._passes(formula) != self.num_layers:
            return False
        from .dropin import MAX_IDS
        return 0 < n_queries and 5 * n_queries <= MAX_IDS

    # ------------------------------------------------------------------ reference entry points
    def forward(self, formula, queries, target_nodes, anchor_ids=None, var_ids=None, q_graphs=None,
                neg_nodes=None, neg_lengths=None):
        if not torch.is_grad_enabled():
            d = self.dropin()
            if d is not None and self._fused_covers(d, formula, len(queries)) and (
                    neg_nodes is None or d.step.uses_chain_dims()):
                return d.forward(formula, queries, target_nodes, anchor_ids, var_ids, q_graphs, neg_nodes, neg_lengths)
        out = self.encode(formula, queries, anchor_ids, var_ids, q_graphs)
        scores = self.score(formula, out, target_nodes, neg_nodes, neg_lengths)
        self._check()
        return scores

    def score_ids(self, formula, anchors, targets, neg=None):
        """forward()'s scores for ids that are on the device already (kg.QuerySet: evaluation.eval_*_queries): anchors
        [B, A] and targets [B] int64, neg None or (ids, offsets [B + 1]) -- every query's negatives, CSR. -> fp32
        [B + total] on the device in forward()'s layout (the B target scores, then the negatives' in CSR order), under
        no_grad. No id and no score visits the host: the template graph depends on the formula and B alone, and the
        module path's ops take the rest as tensors -- one lookup-and-normalise and one ragged cosine over targets and
        negatives together, each row computed as forward()'s module path computes it."""
        with torch.no_grad():
            scores = self._score_ids(formula, anchors, targets, neg)
            self._check()
        return scores

    def _score_ids(self, formula, anchors, targets, neg=None):
        """score_ids' body with gradients enabled (the module path's autograd ops): the differentiable per-formula route
        of margin_loss_ids_by_runs. The caller checks the error word."""
        device = self._device()
        anchors, targets, neg_ids, q_row = _device_ids(anchors, targets, neg, device, len(formula.anchor_modes))
        var_ids, q_graphs = RGCNQueryDataset.get_query_template(formula, anchors.shape[0], self.rel_ids, self.mode_ids)
        out = self.encode(formula, None, anchors, var_ids, q_graphs)
        ids = targets if neg_ids is None else torch.cat([targets, neg_ids])
        return ops.cosine(out, self._target_embeds(ids, formula.target_mode, device), q_row=q_row)

    # ------------------------------------------------------------------ queries of different formulas at once
    MIXED_KEPT = 16         # score_ids_mixed: descriptor blocks kept, one per `formulas` sequence

    def _mixed_passes(self, query_type):
        """encode()'s pass count and the layer of every pass: layer i for pass i, the LAST layer for the last pass"""
        if self.adaptive:
            passes = RGCNQueryDataset.query_diameters[query_type]
            if passes > len(self.layers):
                raise ValueError(f'RGCN is adaptive with {len(self.layers)} layers, but query requires {passes}.')
        else:
            passes = self.num_layers
        return passes, [self.layers[i] for i in range(passes - 1)] + [self.layers[-1]]

    def _mixed_ok(self, formulas, passes):
        """Whether ops.rgcn_scores_mixed covers this model and these formulas: the module path's own configuration
        (`fused`, which also stands for "the library's launches, not a caller's"), a DirectEncoder-style `enc` with `table`
        and `node_maps`, a readout without parameters, at most RGCN_MIX_MAX_PASSES passes, the model on the GPU and the
        library's shape conditions. Everything else is walked run by run (score_ids_by_runs): the same layout, the same
        bits."""
        enc = self.enc
        if not self.fused or self.encode_twice:
            return False
        if not (hasattr(enc, 'table') and getattr(enc, 'node_maps', None) is not None):
            return False
        if self.readout_str not in ('mp', 'sum', 'max') or self._device().type != 'cuda':
            return False
        modes = {m for f in formulas for m in tuple(f.anchor_modes) + (f.target_mode,)}
        if any(enc.table(m).shape[1] != self.emb_dim or enc.table(m).dtype != torch.float32 for m in modes):
            return False
        return ops.rgcn_mixed_supported(self.emb_dim, passes, self.readout_str)

    def _mixed_descriptors(self, formulas):
        """(the kept ops.RgcnMixedDescriptors of `formulas`, or None where the mixed launch does not cover the model; the
        layers of every pass). Kept in self.__dict__['_mixed'] (copies and pickles drop it, _apply resets it), one entry per
        `formulas` sequence, at most MIXED_KEPT of them, the oldest leaving first. An entry is keyed on the identity of
        `formulas`, on what _mixed_ok reads and on data_ptr() of every tensor the block points at -- the block holds
        addresses, not values: an optimizer step keeps it, .to() or a FlatOptimizer that re-homes the parameters makes the
        next call rebuild it."""
        if len(formulas) == 0 or len({f.query_type for f in formulas}) != 1:
            raise ValueError('score_ids_mixed: formulas of one query type')
        passes, layers = self._mixed_passes(formulas[0].query_type)
        kept = self.__dict__.get('_mixed')
        if kept is None:
            kept = self.__dict__['_mixed'] = {}
        entry = kept.get(id(formulas))
        state = (len(formulas), bool(self.fused), bool(self.encode_twice), self.readout_str, passes)
        if entry is not None and entry[1] is formulas and entry[0] == state and (
                entry[2] is None or entry[2].ptrs == tuple(self.enc.table(m).data_ptr() for m in entry[3])):
            return entry[2], layers
        desc, modes = None, []
        if self._mixed_ok(formulas, passes):
            info = ops.template_info(formulas[0].query_type)
            A, V, E = info.num_anchors, info.num_vars, info.num_edges

            def table_of(mode):
                if mode not in modes:
                    modes.append(mode)
                return modes.index(mode)

            recs = np.zeros((len(formulas), _capi.RGCN_MIX_REC_INTS), dtype=np.int32)
            for k, f in enumerate(formulas):
                if len(f.anchor_modes) != A:
                    raise ValueError('formula %s has %d anchor modes, template expects %d' % (f, len(f.anchor_modes), A))
                nodes, rels = f.get_nodes(), f.get_rels()
                recs[k, 0:E] = [self.rel_ids[reverse_relation(rels[info.rel_label[e]])] for e in range(E)]
                recs[k, 3:3 + A] = [table_of(m) for m in f.anchor_modes]
                recs[k, 6:6 + V] = [self.mode_ids[nodes[info.var_node[v]]] for v in range(V)]
                recs[k, 9] = table_of(f.target_mode)
            desc = ops.RgcnMixedDescriptors(formulas[0].query_type, recs, [self.enc.table(m) for m in modes],
                                            self.mode_embeddings.weight.shape[0])
            # (the live tensors the block's addresses are of: the differentiable inputs of margin_loss_ids_mixed)
            desc.live = [self.enc.table(m) for m in modes]
        kept.pop(id(formulas), None)
        while len(kept) >= self.MIXED_KEPT:
            kept.pop(next(iter(kept)))
        kept[id(formulas)] = (state, formulas, desc, modes)
        return desc, layers

    def score_ids_mixed(self, formulas, formula_of, anchors, targets, neg=None):
        """score_ids for queries of DIFFERENT formulas of one query type (kg.MixedQuerySet): `formulas` a sequence of
        Formula of that type, formula_of [B] int64 every query's position in it, the rest as in score_ids over the
        concatenation. -> fp32 [B + total] in forward()'s layout, under no_grad, bit for bit the scores score_ids gives
        run by run. Where the mixed launch covers the model (_mixed_ok) this is ONE ops.rgcn_scores_mixed call -- two
        launches whatever the number of formulas -- and the descriptor block of `formulas` is kept for the next call
        (_mixed_descriptors: pass the SAME sequence object); otherwise the runs of equal formula are walked through
        score_ids (one read of formula_of and the offsets)."""
        if not torch.is_tensor(formula_of) or formula_of.dtype != torch.long or formula_of.dim() != 1:
            raise TypeError('score_ids_mixed: formula_of must be an int64 vector')
        with torch.no_grad():
            desc, layers = self._mixed_descriptors(formulas)
            device = self._device()
            anchors, targets, neg_ids, q_row = _device_ids(anchors, targets, neg, device, len(formulas[0].anchor_modes))
            B = int(targets.shape[0])
            if formula_of.shape[0] != B:
                raise ValueError('score_ids_mixed: formula_of [B]')
            if desc is None:
                return score_ids_by_runs(self, formulas, formula_of.cpu().numpy(), anchors, targets, neg)
            if B == 0:
                return torch.empty(0, dtype=torch.float32, device=device)
            ids = targets if neg_ids is None else torch.cat([targets, neg_ids])
            if q_row is None:
                q_row = torch.arange(B, dtype=torch.long, device=device)
            scores = ops.rgcn_scores_mixed(desc, self.enc.node_maps, self.mode_embeddings.weight,
                                           [(l.basis, l.root, l.bias) for l in layers], self.readout_str,
                                           formula_of.to(device), anchors, ids, q_row, self._error_word(device))
            self._check()
        return scores

    def margin_loss_ids_mixed(self, formulas, formula_of, anchors, targets, neg_ids, margin=1):
        """margin_loss() for B queries of DIFFERENT formulas of one query type with ids on the device (kg.MixedQuerySet.take):
        `formulas` a sequence of Formula of that type (pass the SAME object every time: _mixed_descriptors is keyed on it),
        formula_of [B], anchors [B, A], targets [B] and neg_ids [B] -- one negative per query, as the reference's
        margin_loss draws -- int64. ONE differentiable mixed scoring call over targets ++ neg_ids
        (ops.rgcn_scores_mixed_grad: mpqe_rgcn_fwd_mixed_save, and mpqe_rgcn_bwd_mixed in backward()), then ops.hinge: the
        scalar loss the reference's margin_loss gives for those queries and negatives. The gradients land in .grad of the
        entity tables, mode_embeddings.weight and every layer's basis / root / bias. Where _mixed_ok or
        ops.rgcn_mixed_train_supported says no (learned readouts, fused = False, encode_twice, foreign encoders, other
        shapes) the runs of equal formula are walked through the module path (margin_loss_ids_by_runs)."""
        if not torch.is_tensor(formula_of) or formula_of.dtype != torch.long or formula_of.dim() != 1:
            raise TypeError('margin_loss_ids_mixed: formula_of must be an int64 vector')
        desc, layers = self._mixed_descriptors(formulas)
        distinct = []
        for l in layers:
            if not any(l is d for d in distinct):
                distinct.append(l)
        if desc is None or not ops.rgcn_mixed_train_supported(self.emb_dim, len(layers), self.readout_str, len(distinct)):
            return margin_loss_ids_by_runs(self, formulas, formula_of, anchors, targets, neg_ids, margin)
        device = self._device()
        B = int(targets.shape[0])
        rows = torch.arange(B + 1, dtype=torch.long, device=device)
        neg_ids = neg_ids.to(device).reshape(-1)
        if formula_of.shape[0] != B or neg_ids.shape[0] != B:
            raise ValueError('margin_loss_ids_mixed: formula_of [B], neg_ids [B]')
        anchors, targets, neg_ids, _ = _device_ids(anchors, targets, (neg_ids, rows), device, len(formulas[0].anchor_modes))
        layer_of_pass = [[l is d for d in distinct].index(True) for l in layers]
        # (the fused step's error word where the model has one: the word the flat optimizer's guard reads, so that the
        # update after a flagged window is refused on the device, as after a flagged margin_loss)
        step = self.dropin()
        err = step.step.err if step is not None else self._error_word(device)
        scores = ops.rgcn_scores_mixed_grad(desc, desc.live, self.mode_embeddings.weight,
                                            [(l.basis, l.root, l.bias) for l in distinct], layer_of_pass, self.enc.node_maps,
                                            self.readout_str, formula_of.to(device).contiguous(), anchors,
                                            torch.cat([targets, neg_ids]), rows, err)
        # (_check() reads self._err and the encoder's word; the call above wrote `err`, which is the step's word where there
        # is a step and self._err otherwise -- so the step's word is read here and _check() covers the rest)
        if self.validate and step is not None:
            ops.raise_on_flags(err)
        self._check()
        return ops.hinge(scores[:B], scores[B:], margin)

    # ------------------------------------------------------------------ answering a query (no counterpart in the reference)
    def _query_embeddings(self, formula, queries, anchor_ids, var_ids, q_graphs):
        d = self.dropin()
        if d is not None and self._fused_covers(d, formula, len(queries)):
            q = d.query_embeddings(formula, queries, anchor_ids, var_ids, q_graphs)
            if q is not None:
                return q
        return self.encode(formula, queries, anchor_ids, var_ids, q_graphs)

    def _rank_all(self, formula, queries, target_nodes, exclude, k, anchor_ids, var_ids, q_graphs):
        def operands(n):
            q = self._query_embeddings(formula, queries, anchor_ids, var_ids, q_graphs)
            return q, self.enc.table(formula.target_mode).detach()[:n]
        return self._rank_rows(formula, queries, target_nodes, exclude, k, operands)

    def _rank_operands_ids(self, formula, anchors, n):
        """rank_ids' operands: the module path's query embeddings of device anchors (as _score_ids encodes them) and the
        target mode's first n rows"""
        var_ids, q_graphs = RGCNQueryDataset.get_query_template(formula, anchors.shape[0], self.rel_ids, self.mode_ids)
        q = self.encode(formula, None, anchors, var_ids, q_graphs)
        return q, self.enc.table(formula.target_mode).detach()[:n], 'cosine'

    def _embed_mixed(self, formulas, formula_of, anchors):
        """rank_ids_mixed's query embeddings [B, D] in one ops.rgcn_embed_mixed call, or None where _mixed_ok says the
        mixed launch does not cover the model"""
        desc, layers = self._mixed_descriptors(formulas)
        if desc is None:
            return None
        return ops.rgcn_embed_mixed(desc, self.enc.node_maps, self.mode_embeddings.weight,
                                    [(l.basis, l.root, l.bias) for l in layers], self.readout_str, formula_of, anchors,
                                    self._error_word(self._device()))

    def answer(self, formula, queries, k=10, exclude=None, anchor_ids=None, var_ids=None, q_graphs=None):
        """The k entities of formula.target_mode the model proposes for each query, best first:
        (ids [B, k] int64 global entity ids, scores [B, k] float32), -1 / -inf past the last eligible entity. The score is
        the one forward() gives a candidate. `exclude`: one list of entity ids per query that must not be returned.
        Every entity of the mode is scored (mpqe_rank_entities); k <= ops.RANK_MAX_K."""
        if k < 1:
            raise ValueError('answer: k must be at least 1')
        with torch.no_grad():
            ids, scores, _ = self._rank_all(formula, queries, None, exclude, k, anchor_ids, var_ids, q_graphs)
        return ids, scores

    def rank_targets(self, formula, queries, target_nodes=None, exclude=None, anchor_ids=None, var_ids=None,
                     q_graphs=None):
        """ranks [B] int64: 1 + the number of entities of formula.target_mode, other than the target and those in
        `exclude`, that the model places before each query's target (default: query.target_node); ties go to the entity
        with the smaller table row. The target is never excluded, listed or not (the filtered setting passes every known
        answer)."""
        if target_nodes is None:
            target_nodes = [query.target_node for query in queries]
        with torch.no_grad():
            _, _, rank = self._rank_all(formula, queries, target_nodes, exclude, 0, anchor_ids, var_ids, q_graphs)
        return rank

    def sample_negatives(self, formula, queries, hard_negatives=False):
        """reference: model.py:466-476 (same python `random` stream, so the same draws)."""
        return sample_negatives(self.graph, formula, queries, hard_negatives)

    def margin_loss(self, formula, queries, anchor_ids=None, var_ids=None, q_graphs=None,
                    hard_negatives=False, margin=1):
        d = self.dropin()
        if d is not None and self._fused_covers(d, formula, len(queries)):
            return d.margin_loss(formula, queries, anchor_ids, var_ids, q_graphs, hard_negatives, margin)
        neg_nodes = self.sample_negatives(formula, queries, hard_negatives)
        targets = [query.target_node for query in queries]
        if self.encode_twice:
            affs = self.forward(formula, queries, targets, anchor_ids, var_ids, q_graphs)
            neg_affs = self.forward(formula, queries, neg_nodes, anchor_ids, var_ids, q_graphs)
        else:
            out = self.encode(formula, queries, anchor_ids, var_ids, q_graphs)
            affs = self.score(formula, out, targets)
            neg_affs = self.score(formula, out, neg_nodes)
        loss = ops.hinge(affs, neg_affs, margin)

        if isinstance(self.readout, nn.Module) and self.weight_decay > 0:
            # (reference model.py:486-490: l2_reg = sum of torch.norm(param) -- on the library's kernel, the one the fused step uses)
            loss = loss + self.weight_decay * ops.l2_norms(list(self.readout.parameters()))
        self._check()
        return loss


def _mlp(layers, x):
    """nn.Sequential(Linear, ReLU, Linear) of the readouts through ops.linear."""
    h = ops.linear(x.contiguous(), layers[0].weight, layers[0].bias, relu=True)
    return ops.linear(h, layers[2].weight, layers[2].bias)


class MLPReadout(nn.Module):
    """reference: model.py:497-515. Linear-ReLU-Linear per node, then the scatter reduction kernel. The nn.Linear
    modules hold the parameters (state_dict keys layers.0 / layers.2, the reference's init); the arithmetic runs on the
    library's own MFMA tiles (ops.linear: mpqe_linear_fwd / bwd, the ReLU fused into the first product's epilogue)."""

    def __init__(self, input_dim, output_dim, scatter_fn):
        super(MLPReadout, self).__init__()
        self.layers = nn.Sequential(nn.Linear(in_features=input_dim, out_features=output_dim),
                                    nn.ReLU(),
                                    nn.Linear(in_features=output_dim, out_features=output_dim))
        self.scatter_fn = scatter_fn

    def forward(self, embs, batch_idx, batch_size=None, **kwargs):
        x = _mlp(self.layers, embs)
        x = self.scatter_fn(x, batch_idx, dim=0, dim_size=batch_size)
        if isinstance(x, tuple):
            x = x[0]
        return x


class TargetMLPReadout(nn.Module):
    """reference: model.py:518-553."""

    def __init__(self, dim, scatter_fn):
        super(TargetMLPReadout, self).__init__()
        self.layers = nn.Sequential(nn.Linear(in_features=2 * dim, out_features=dim),
                                    nn.ReLU(),
                                    nn.Linear(in_features=dim, out_features=dim))
        self.scatter_fn = scatter_fn

    def forward(self, embs, batch_idx, batch_size, num_nodes, num_anchors, **kwargs):
        keep = [n for n in range(num_nodes) if n != num_anchors]
        batch_idx = batch_idx.reshape(batch_size, -1)[:, keep].reshape(-1)
        embs = embs.reshape(batch_size, num_nodes, -1)
        non_targets = embs[:, keep]
        targets = embs[:, num_anchors:num_anchors + 1].expand_as(non_targets)
        x = torch.cat((targets, non_targets), dim=-1)
        x = x.reshape(batch_size * (num_nodes - 1), -1).contiguous()
        x = _mlp(self.layers, x)
        x = self.scatter_fn(x, batch_idx, dim=0, dim_size=batch_size)
        if isinstance(x, tuple):
            x = x[0]
        return x


# ------------------------------------------------------------------------------------------------ the GQE baseline
def _anchor_ids(queries, slot):
    return [query.anchor_nodes[slot] for query in queries]


def _device_ids(anchors, targets, neg, device, num_anchors):
    """score_ids' operands checked and on `device`: (anchors [B, A], targets [B], negative ids [total] or None, the row map
    [B + total] of forward()'s ragged layout -- arange(B), then query i repeated once per negative -- or None). The
    negatives' count is the id tensor's length, so nothing is read back."""
    def ids(t, what):
        if not torch.is_tensor(t) or t.dtype != torch.long:
            raise TypeError('score_ids: %s must be an int64 tensor' % what)
        return t.to(device).contiguous()
    anchors, targets = ids(anchors, 'anchors'), ids(targets, 'targets')
    B = int(targets.shape[0])
    if anchors.dim() != 2 or targets.dim() != 1 or tuple(anchors.shape) != (B, num_anchors):
        raise ValueError('score_ids: anchors [B, %d] and targets [B]' % num_anchors)
    if neg is None:
        return anchors, targets, None, None
    neg_ids, offsets = ids(neg[0], 'the negatives'), ids(neg[1], 'the negatives\' offsets')
    if neg_ids.dim() != 1 or offsets.dim() != 1 or offsets.shape[0] != B + 1:
        raise ValueError('score_ids: neg = (ids [total], offsets [B + 1])')
    rows = torch.arange(B, dtype=torch.long, device=device)
    q_row = torch.cat([rows, torch.repeat_interleave(rows, offsets[1:] - offsets[:-1], output_size=int(neg_ids.shape[0]))])
    return anchors, targets, neg_ids, q_row


def formula_runs(formula_of):
    """[(formula index, lo, hi)] of the maximal stretches of equal entries of a host int vector"""
    fo = np.asarray(formula_of, dtype=np.int64)
    if fo.shape[0] == 0:
        return []
    cuts = np.concatenate([[0], np.nonzero(fo[1:] != fo[:-1])[0] + 1, [fo.shape[0]]])
    return [(int(fo[lo]), int(lo), int(hi)) for lo, hi in zip(cuts[:-1], cuts[1:])]


def score_ids_by_runs(model, formulas, formula_of_host, anchors, targets, neg=None, offsets_host=None):
    """model.score_ids over every run of equal formula of a concatenation, the scores put back in forward()'s layout of the
    whole: [B] targets, then the negatives in CSR order. For a model without a mixed launch (RGCNEncoderDecoder) and for
    the formulas the fused GQE kernel does not cover. offsets_host: the host mirror of neg[1] (read from the device
    otherwise)."""
    B = int(targets.shape[0])
    if neg is not None and offsets_host is None:
        offsets_host = neg[1].cpu().numpy()
    total = 0 if neg is None else int(neg[0].shape[0])
    out = None
    for f, lo, hi in formula_runs(formula_of_host):
        if not 0 <= f < len(formulas):
            raise IndexError('formula index %d outside the %d formulas' % (f, len(formulas)))
        sub = None
        if neg is not None:
            a, b = int(offsets_host[lo]), int(offsets_host[hi])
            sub = (neg[0][a:b], neg[1][lo:hi + 1] - a)
        s = model.score_ids(formulas[f], anchors[lo:hi], targets[lo:hi], neg=sub)
        if out is None:
            out = torch.empty(B + total, dtype=torch.float32, device=s.device)
        out[lo:hi] = s[:hi - lo]
        if neg is not None:
            out[B + a:B + b] = s[hi - lo:]
    if out is None:
        out = torch.empty(0, dtype=torch.float32, device=targets.device)
    return out


def rank_ids_by_runs(model, formulas, formula_of_host, anchors, targets, exclude=None, k=0):
    """model.rank_ids over every run of equal formula of a concatenation -> (ranks [B], top-k ids [B, k] or None, top-k
    scores) of the whole. exclude: a kg.KGAnswersMixed with its bitmaps, or None; a run's answers are the rows of its
    bitmaps cut to the target mode's words. rank_ids_mixed's fallback (learned readouts, chain types of the GQE model,
    models without a mixed embedding) and its oracle."""
    from .kg import KGAnswers, _words
    B = int(targets.shape[0])
    ranks, ids, scores = torch.empty(B, dtype=torch.int64, device=targets.device), None, None
    for f, lo, hi in formula_runs(formula_of_host):
        if not 0 <= f < len(formulas):
            raise IndexError('formula index %d outside the %d formulas' % (f, len(formulas)))
        sub = None
        if exclude is not None:
            index, mode = exclude.index, formulas[f].target_mode
            n = int(index.mode_rows[index.mode_index[mode]])
            sub = KGAnswers(index, formulas[f], mode, n, exclude.bits[lo:hi, :_words(n)].contiguous(), None,
                            exclude.counts[:, lo:hi].contiguous())
        r, i, s = model.rank_ids(formulas[f], anchors[lo:hi], targets[lo:hi], sub, k)
        ranks = ranks.to(r.device)
        ranks[lo:hi] = r
        if i is not None:
            if ids is None:
                ids = torch.empty((B, k), dtype=torch.int64, device=i.device)
                scores = torch.empty((B, k), dtype=torch.float32, device=i.device)
            ids[lo:hi], scores[lo:hi] = i, s
    return ranks, ids, scores


def margin_loss_ids_by_runs(model, formulas, formula_of, anchors, targets, neg_ids, margin=1):
    """margin_loss_ids_mixed of either model without the mixed launch: every run of equal formula through the
    differentiable per-formula route (model._score_ids -- QueryEncoderDecoder: ops.gqe_scores where the fused kernel
    covers the formula, the composed ops otherwise; RGCNEncoderDecoder: the module path's ops), the scores put back in
    forward()'s layout of the whole, one hinge. Its fallback, its oracle and the other side of
    tools/gqe_mixed_train_bench.py and tools/rgcn_mixed_train_bench.py (one read of formula_of)."""
    device = model._device()
    B = int(targets.shape[0])
    anchors, targets, neg_ids = anchors.to(device), targets.to(device), neg_ids.to(device).reshape(-1)
    pos, negs = [], []
    for f, lo, hi in formula_runs(formula_of.cpu().numpy()):
        if not 0 <= f < len(formulas):
            raise IndexError('formula index %d outside the %d formulas' % (f, len(formulas)))
        off = torch.arange(hi - lo + 1, dtype=torch.long, device=device)
        s = model._score_ids(formulas[f], anchors[lo:hi], targets[lo:hi], (neg_ids[lo:hi], off))
        pos.append(s[:hi - lo])
        negs.append(s[hi - lo:])
    model._check()
    scores = torch.cat(pos + negs)
    return ops.hinge(scores[:B], scores[B:], margin)


def gqe_plan(formula):
    """(form, [(anchor slot or None = the target side, mode, [(relation, transposed)])], intersection mode or None,
    [(relation, transposed)] after the intersection, mode of the other side): model.py:78-116 as data."""
    from .graph import reverse_relation as rev
    qt, rels = formula.query_type, formula.rels
    if qt in ('1-chain', '2-chain', '3-chain'):
        return 0, [(None, formula.target_mode, [(tuple(r), False) for r in rels])], None, [], formula.anchor_modes[0]
    if qt == '3-chain_inter':
        branches = [(0, formula.anchor_modes[0], [(rev(rels[1][0]), True)]),
                    (1, formula.anchor_modes[1], [(rev(rels[1][1]), True)])]
        return 1, branches, rels[0][-1], [(rev(rels[0]), True)], formula.target_mode
    if qt not in ('2-inter', '3-inter', '3-inter_chain'):
        raise ValueError('unknown query type %r' % (qt,))
    branches = [(0, formula.anchor_modes[0], [(rev(rels[0]), True)])]
    if len(rels[1]) == 2:
        branches.append((1, formula.anchor_modes[1], [(rev(r), True) for r in rels[1][::-1]]))
    else:
        branches.append((1, formula.anchor_modes[1], [(rev(rels[1]), True)]))
    if qt == '3-inter':
        branches.append((2, formula.anchor_modes[2], [(rev(rels[2]), True)]))
    return 1, branches, formula.target_mode, [], formula.target_mode


class QueryEncoderDecoder(nn.Module, _EntityRanking):
    """reference: QueryEncoderDecoder, model.py:57-134 -- GQE: a path decoder and an intersection decoder over entity
    embeddings. Same constructor, forward() / margin_loss() signatures and state_dict keys (enc.*, path_dec.*,
    inter_dec.*).

    fused = True: forward() is ONE ops.gqe_scores call (mpqe_gqe_fwd / mpqe_gqe_bwd, csrc/gqe.hip) and margin_loss() one
    for targets and negatives together. Taken with a DirectEncoder that has node_maps, a BilinearMetapathDecoder,
    TransEMetapathDecoder or BilinearDiagMetapathDecoder (the path operator and the parameters come from the decoder's
    type: matrices `mats`, or vectors `vecs` that translate / scale), a SetIntersection / SimpleSetIntersection, parameters on the GPU and a shape the kernel covers (one D for every mode,
    a multiple of 16 up to 256). Everything else -- and fused = False -- takes the composed path: the decoders' own
    forward / project, one library call per product.

    answer() / rank_targets() (no counterpart in the reference) score every entity of the target mode in one
    ops.rank_entities call, as on RGCNEncoderDecoder. An intersection formula's B query embeddings come from
    ops.gqe_embed (mpqe_gqe_embed: the forward's P side alone) and are ranked against the mode's table. In a chain formula
    the rows that pass through the matrices are the candidates, and they depend on the formula alone: the mode's table is
    projected ONCE ([n, D], not once per query) and the B normalised anchors are ranked against it -- by the cosine, or by
    the dot product under the diagonal decoder, whose chains forward() scores that way. In eval() mode that
    projection is kept for the next call (one entry, self.__dict__['_cand']: copies and pickles drop it), keyed on the
    chain's relations, the target mode, the device and data_ptr() / _version of the table and of every matrix or vector
    used; in
    train() mode it is always recomputed. Code that writes parameters through raw pointers (no version bump) must switch
    to train() or set model.__dict__['_cand'] = None."""

    MIXED_KEPT = 16         # score_ids_mixed: descriptor blocks kept, one per `formulas` sequence

    def __init__(self, graph, enc, path_dec, inter_dec):
        super(QueryEncoderDecoder, self).__init__()
        self.enc = enc
        self.path_dec = path_dec
        self.inter_dec = inter_dec
        self.graph = graph
        self.fused = True
        # one 4-byte D2H read per call to turn a bad id into IndexError (see ops.raise_on_flags)
        self.validate = True
        self._err = None

    def __getstate__(self):
        state = self.__dict__.copy()
        state['_err'] = None
        state['_row_ids'] = None        # (what answer() caches on the device: the row -> id maps, a chain's projected candidates)
        state['_maps_np'] = None
        state['_cand'] = None
        state['_mixed'] = None          # (score_ids_mixed's descriptor block: device addresses)
        return state

    def _apply(self, fn, *args, **kwargs):
        # (.to() / .cuda() / .float(): the parameters move)
        out = super(QueryEncoderDecoder, self)._apply(fn, *args, **kwargs)
        self.__dict__['_row_ids'] = None
        self.__dict__['_maps_np'] = None
        self.__dict__['_cand'] = None
        self.__dict__['_mixed'] = None
        return out

    # ------------------------------------------------------------------ helpers
    def _device(self):
        return next(self.parameters()).device

    def _error_word(self, device):
        if self._err is None or self._err.device != device:
            self._err = ops.new_error_word(device)
        return self._err

    def _check(self):
        if self.validate:
            for err in (self._err, getattr(self.enc, '_err', None)):
                if err is not None:
                    ops.raise_on_flags(err)

    def _plan(self, formula):
        return gqe_plan(formula)

    def _path_kind(self):
        """(path operator, the decoder's parameters by relation, chain score) from the type of path_dec, or None for a
        decoder the fused kernel does not know."""
        from .decoders import BilinearDiagMetapathDecoder, BilinearMetapathDecoder, TransEMetapathDecoder
        kind = type(self.path_dec)
        if kind is BilinearMetapathDecoder:
            return 'matrix', self.path_dec.mats, 'cosine'
        if kind in (TransEMetapathDecoder, BilinearDiagMetapathDecoder):
            return self.path_dec.op, self.path_dec.vecs, self.path_dec.score
        return None

    def _plan_score(self, plan):
        """How forward() scores this plan's pairs: the decoder's own score on a chain (model.py:80-83 hands a chain to
        path_dec.forward), the model's cosine on every intersection form (model.py:104, 115)."""
        return getattr(self.path_dec, 'score', 'cosine') if plan[0] == 0 else 'cosine'

    def _fused_ok(self, plan):
        from .decoders import SetIntersection, SimpleSetIntersection
        enc = self.enc
        if not self.fused or not (hasattr(enc, 'table') and getattr(enc, 'node_maps', None) is not None):
            return False
        kind = self._path_kind()
        if kind is None or type(self.inter_dec) not in (SetIntersection, SimpleSetIntersection):
            return False
        if self._device().type != 'cuda':
            return False
        op, path, _ = kind
        form, branches, imode, tail, emode = plan
        dims = {enc.table(m).shape[1] for _, m, _ in branches} | {enc.table(emode).shape[1]}
        used = [path[r] for _, _, steps in branches for r, _ in steps] + [path[r] for r, _ in tail]
        mats = []
        if imode is not None and isinstance(self.inter_dec, SetIntersection):
            mats += [self.inter_dec.pre_mats[imode], self.inter_dec.post_mats[imode]]
        if len(dims) != 1:
            return False
        D = next(iter(dims))
        want = (D, D) if op == 'matrix' else (D,)
        return (ops.gqe_supported(D) and all(tuple(p.shape) == want for p in used)
                and all(tuple(m.shape) == (D, D) for m in mats))

    def _programme(self, plan, shared=None):
        """(programme of mpqe_gqe_fwd / mpqe_gqe_embed, the modes of its tables, its matrices / vectors) of one plan.
        shared: (modes, mats, {id(parameter): index}) that several programmes number their tables and parameters in
        (score_ids_mixed); they grow in place."""
        from .decoders import SetIntersection
        form, branches, imode, tail, emode = plan
        op, path, _ = self._path_kind()
        modes, mats, mat_ids = ([], [], {}) if shared is None else shared

        def table_of(mode):
            if mode not in modes:
                modes.append(mode)
            return modes.index(mode)

        def mat_of(param):
            if id(param) not in mat_ids:
                mat_ids[id(param)] = len(mats)
                mats.append(param)
            return mat_ids[id(param)]

        prog_branches = [(table_of(m), [(mat_of(path[r]), t) for r, t in steps]) for _, m, steps in branches]
        prog_tail = [(mat_of(path[r]), t) for r, t in tail]
        pre = post = -1
        if imode is not None and isinstance(self.inter_dec, SetIntersection):
            pre, post = mat_of(self.inter_dec.pre_mats[imode]), mat_of(self.inter_dec.post_mats[imode])
        agg = self.inter_dec.agg_kind if imode is not None else 'mean'
        prog = ops.gqe_programme(form, prog_branches, table_of(emode), agg, pre, post, prog_tail, op=op,
                                 score=self._plan_score(plan))
        return prog, modes, mats

    def _fused_scores(self, formula, queries, target_nodes, neg_nodes, neg_lengths, plan):
        form, branches, imode, tail, emode = plan
        enc, device = self.enc, self._device()
        B = len(queries)
        tnodes = list(target_nodes) + (list(neg_nodes) if neg_nodes is not None else [])
        n = len(tnodes)
        lengths = np.asarray(neg_lengths, dtype=np.int64) if neg_nodes is not None else np.zeros(B, dtype=np.int64)
        if neg_nodes is not None and (lengths.shape[0] != B or int(lengths.sum()) != n - B or (lengths < 0).any()):
            raise ValueError('neg_lengths must hold one length per query and sum to len(neg_nodes)')
        prog, modes, mats = self._programme(plan)
        anchors = [_anchor_ids(queries, slot) for slot, _, _ in branches if slot is not None]
        qrow = neg_off = None
        if form == 0:
            p_ids = np.asarray(tnodes, dtype=np.int64).reshape(1, n)
            e_ids = np.asarray(_anchor_ids(queries, 0), dtype=np.int64)
            qrow = np.concatenate([np.arange(B, dtype=np.int64), np.repeat(np.arange(B, dtype=np.int64), lengths)])
        else:
            p_ids = np.asarray(anchors, dtype=np.int64).reshape(len(branches), B)
            e_ids = np.asarray(tnodes, dtype=np.int64)
            if n > B:
                neg_off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        # (one host-to-device copy for all the integer inputs of the call)
        parts = [p_ids.reshape(-1), e_ids] + [a for a in (qrow, neg_off) if a is not None]
        flat = torch.from_numpy(np.concatenate(parts)).to(device)
        cuts = np.cumsum([0] + [p.shape[0] for p in parts])
        views = [flat[cuts[k]:cuts[k + 1]] for k in range(len(parts))]
        p_dev, e_dev = views[0].view(p_ids.shape), views[1]
        rest = views[2:]
        q_dev = rest.pop(0) if qrow is not None else None
        o_dev = rest.pop(0) if neg_off is not None else None
        return ops.gqe_scores(prog, [enc.table(m) for m in modes], mats, enc.node_maps, p_dev, e_dev, q_dev, o_dev, n,
                              self._error_word(device))

    def score_ids(self, formula, anchors, targets, neg=None):
        """forward()'s scores for ids that are on the device already (kg.QuerySet: evaluation.eval_*_queries): anchors
        [B, A] and targets [B] int64, neg None or (ids, offsets [B + 1]) -- every query's negatives, CSR. -> fp32
        [B + total] on the device in forward()'s layout, under no_grad. The integer operands of ops.gqe_scores are put
        together with tensor ops -- the launch is _fused_scores', so the bits are forward()'s; where the fused kernel does
        not cover the model the composed path runs on the same tensors. No id and no score visits the host."""
        with torch.no_grad():
            scores = self._score_ids(formula, anchors, targets, neg)
            self._check()
        return scores

    def _score_ids(self, formula, anchors, targets, neg=None):
        """score_ids' scores without its no_grad and its check: differentiable w.r.t. the parameters (ops.gqe_scores where
        the fused kernel covers the formula, the composed ops otherwise)"""
        plan = self._plan(formula)
        form, branches, imode, tail, emode = plan
        device = self._device()
        anchors, targets, neg_ids, q_row = _device_ids(anchors, targets, neg, device, len(formula.anchor_modes))
        B = int(targets.shape[0])
        tnodes = targets if neg_ids is None else torch.cat([targets, neg_ids])
        n = int(tnodes.shape[0])
        if not self._fused_ok(plan):
            return self._composed_ids(formula, anchors, tnodes, q_row, plan)
        prog, modes, mats = self._programme(plan)
        qrow = neg_off = None
        if form == 0:
            p_ids, e_ids = tnodes.reshape(1, n), anchors[:, 0].contiguous()
            qrow = q_row if q_row is not None else torch.arange(B, dtype=torch.long, device=device)
        else:
            slots = [slot for slot, _, _ in branches if slot is not None]
            p_ids, e_ids = anchors[:, slots].t().contiguous(), tnodes
            if n > B:
                neg_off = neg[1].to(device).contiguous()
        return ops.gqe_scores(prog, [self.enc.table(m) for m in modes], mats, self.enc.node_maps, p_ids, e_ids, qrow, neg_off,
                              n, self._error_word(device))

    def _mixed_descriptors(self, formulas):
        """(the kept ops.GqeMixedDescriptors of `formulas`, or None where the fused kernel does not cover every formula;
        the first formula's plan). Kept in self.__dict__['_mixed'] (copies and pickles drop it), one entry per `formulas`
        sequence -- an evaluation walks the seven query types in turn --, at most MIXED_KEPT of them, the oldest leaving
        first. An entry is keyed on the identity of `formulas`, `fused` and data_ptr() of every parameter (the tables among
        them): the block holds addresses, not values, so an optimizer step keeps it, and a call that finds it does no work
        per formula."""
        key = (len(formulas), bool(self.fused), tuple(p.data_ptr() for p in self.parameters()))
        kept = self.__dict__.get('_mixed')
        if kept is None:
            kept = self.__dict__['_mixed'] = {}
        entry = kept.get(id(formulas))
        if entry is not None and entry[0] == key and entry[1] is formulas:
            return entry[2], entry[3]
        if len(formulas) == 0 or len({f.query_type for f in formulas}) != 1:
            raise ValueError('score_ids_mixed: formulas of one query type')
        plans = [self._plan(f) for f in formulas]
        desc = None
        same = len({(plan[0], len(plan[1]), tuple(len(steps) for _, _, steps in plan[1]), len(plan[3]), plan[2] is None)
                    for plan in plans}) == 1
        if same and all(self._fused_ok(plan) for plan in plans):
            shared = ([], [], {})
            progs = np.stack([self._programme(plan, shared)[0] for plan in plans])
            desc = ops.GqeMixedDescriptors(progs, [self.enc.table(m) for m in shared[0]], shared[1])
            # (the live tensors the block's addresses are of: the differentiable inputs of margin_loss_ids_mixed)
            desc.live = ([self.enc.table(m) for m in shared[0]], list(shared[1]))
        kept.pop(id(formulas), None)
        while len(kept) >= self.MIXED_KEPT:
            kept.pop(next(iter(kept)))
        kept[id(formulas)] = (key, formulas, desc, plans[0])
        return desc, plans[0]

    def score_ids_mixed(self, formulas, formula_of, anchors, targets, neg=None):
        """score_ids for queries of DIFFERENT formulas of one query type (kg.MixedQuerySet): `formulas` a sequence of
        Formula of that type, formula_of [B] int64 every query's position in it, the rest as in score_ids over the
        concatenation. -> fp32 [B + total] in forward()'s layout, under no_grad, bit for bit the scores score_ids gives
        run by run. Where the fused kernel covers every formula this is ONE ops.gqe_scores_mixed launch, and the
        descriptor block of `formulas` is kept for the next call (_mixed_descriptors: pass the SAME sequence object);
        otherwise the runs of equal formula are walked through score_ids (one read of formula_of and the offsets)."""
        if not torch.is_tensor(formula_of) or formula_of.dtype != torch.long or formula_of.dim() != 1:
            raise TypeError('score_ids_mixed: formula_of must be an int64 vector')
        with torch.no_grad():
            desc, (form, branches, imode, tail, emode) = self._mixed_descriptors(formulas)
            device = self._device()
            anchors, targets, neg_ids, q_row = _device_ids(anchors, targets, neg, device, len(formulas[0].anchor_modes))
            B = int(targets.shape[0])
            if formula_of.shape[0] != B:
                raise ValueError('score_ids_mixed: formula_of [B]')
            if desc is None:
                return self._mixed_by_runs(formulas, formula_of, anchors, targets, neg)
            formula_of = formula_of.to(device).contiguous()
            tnodes = targets if neg_ids is None else torch.cat([targets, neg_ids])
            n = int(tnodes.shape[0])
            qrow = neg_off = None
            if form == 0:
                p_ids, e_ids = tnodes.reshape(1, n), anchors[:, 0].contiguous()
                qrow = q_row if q_row is not None else torch.arange(B, dtype=torch.long, device=device)
            else:
                slots = [slot for slot, _, _ in branches if slot is not None]
                p_ids, e_ids = anchors[:, slots].t().contiguous(), tnodes
                if n > B:
                    neg_off = neg[1].to(device).contiguous()
            scores = ops.gqe_scores_mixed(desc, self.enc.node_maps, formula_of, p_ids, e_ids, qrow, neg_off, n,
                                          self._error_word(device))
            self._check()
        return scores

    def margin_loss_ids_mixed(self, formulas, formula_of, anchors, targets, neg_ids, margin=1):
        """margin_loss() for B queries of DIFFERENT formulas of one query type with ids on the device (kg.MixedQuerySet.take):
        `formulas` a sequence of Formula of that type (pass the SAME object every time: _mixed_descriptors is keyed on it),
        formula_of [B], anchors [B, A], targets [B] and neg_ids [B] -- one negative per query, as the reference's
        margin_loss draws -- int64. ONE differentiable mixed scoring call over targets ++ neg_ids
        (ops.gqe_scores_mixed_grad: mpqe_gqe_fwd_mixed_save, and mpqe_gqe_bwd_mixed in backward()), then ops.hinge: the
        scalar loss the reference's margin_loss gives for those queries and negatives. Where the fused kernel does not
        cover every formula (fused = False, a D it does not take, foreign decoders) the runs of equal formula are walked
        through the per-formula route (margin_loss_ids_by_runs)."""
        if not torch.is_tensor(formula_of) or formula_of.dtype != torch.long or formula_of.dim() != 1:
            raise TypeError('margin_loss_ids_mixed: formula_of must be an int64 vector')
        desc, (form, branches, imode, tail, emode) = self._mixed_descriptors(formulas)
        if desc is None:
            return margin_loss_ids_by_runs(self, formulas, formula_of, anchors, targets, neg_ids, margin)
        device = self._device()
        B = int(targets.shape[0])
        rows = torch.arange(B + 1, dtype=torch.long, device=device)
        neg_ids = neg_ids.to(device).reshape(-1)
        if formula_of.shape[0] != B or neg_ids.shape[0] != B:
            raise ValueError('margin_loss_ids_mixed: formula_of [B], neg_ids [B]')
        anchors, targets, neg_ids, _ = _device_ids(anchors, targets, (neg_ids, rows), device, len(formulas[0].anchor_modes))
        formula_of = formula_of.to(device).contiguous()
        tnodes = torch.cat([targets, neg_ids])
        qrow = neg_off = None
        if form == 0:
            p_ids, e_ids = tnodes.reshape(1, 2 * B), anchors[:, 0].contiguous()
            qrow = torch.cat([rows[:B], rows[:B]])
        else:
            slots = [slot for slot, _, _ in branches if slot is not None]
            p_ids, e_ids, neg_off = anchors[:, slots].t().contiguous(), tnodes, rows
        scores = ops.gqe_scores_mixed_grad(desc, desc.live[0], desc.live[1], self.enc.node_maps, formula_of, p_ids, e_ids,
                                           qrow, neg_off, 2 * B, self._error_word(device))
        self._check()
        return ops.hinge(scores[:B], scores[B:], margin)

    def _mixed_by_runs(self, formulas, formula_of, anchors, targets, neg):
        """score_ids_mixed without the mixed launch: every run of equal formula through score_ids, put back in forward()'s
        layout of the whole"""
        return score_ids_by_runs(self, formulas, formula_of.cpu().numpy(), anchors, targets, neg)

    def _composed_ids(self, formula, anchors, tnodes, q_row, plan):
        """_composed_scores on id tensors (enc(ids, mode) takes them)"""
        form, branches, imode, tail, emode = plan
        target_embeds = self.enc(tnodes, formula.target_mode)
        if form == 0:
            first = self.enc(anchors[:, 0], formula.anchor_modes[0])
            if hasattr(self.path_dec, 'vecs'):
                return self.path_dec(target_embeds, first if q_row is None else first[:, q_row],
                                     [rel for rel, _ in branches[0][2]])
            act = target_embeds.t()
            for rel, _ in branches[0][2]:
                act = ops.linear(act, self.path_dec.mats[rel].t())
            return ops.cosine(first.t(), act, q_row=q_row)
        embeds = []
        for slot, mode, steps in branches:
            e = self.enc(anchors[:, slot], mode)
            for rel, _ in steps:
                e = self.path_dec.project(e, rel)
            embeds.append(e)
        q = self.inter_dec(embeds[0], embeds[1], imode, *embeds[2:])
        for rel, _ in tail:
            q = self.path_dec.project(q, rel)
        return ops.cosine(q.t(), target_embeds.t(), q_row=q_row)

    # ------------------------------------------------------------------ the composed path (model.py:70-116 op by op)
    def _composed_scores(self, formula, queries, target_nodes, neg_nodes, neg_lengths, plan):
        form, branches, imode, tail, emode = plan
        B = len(queries)
        q_row = None
        if neg_nodes is not None:
            target_nodes = list(target_nodes) + list(neg_nodes)
            lengths = torch.as_tensor(neg_lengths, dtype=torch.long)
            q_row = torch.cat([torch.arange(B), torch.repeat_interleave(torch.arange(B), lengths)]).to(self._device())
        target_embeds = self.enc(target_nodes, formula.target_mode)
        if form == 0:
            anchors = self.enc(_anchor_ids(queries, 0), formula.anchor_modes[0])
            if hasattr(self.path_dec, 'vecs'):
                # (the vector decoders' own forward: plain tensor ops, one anchor column per scored pair)
                return self.path_dec(target_embeds, anchors if q_row is None else anchors[:, q_row],
                                     [rel for rel, _ in branches[0][2]])
            act = target_embeds.t()
            for rel, _ in branches[0][2]:
                act = ops.linear(act, self.path_dec.mats[rel].t())
            return ops.cosine(anchors.t(), act, q_row=q_row)
        return ops.cosine(self._composed_query(queries, plan).t(), target_embeds.t(), q_row=q_row)

    def _composed_query(self, queries, plan, anchors=None):
        """[D, B]: an intersection formula's query embeddings from the decoders' own pieces (model.py:84-116). anchors: the
        anchor ids [B, A] on the device in place of `queries`."""
        form, branches, imode, tail, emode = plan
        embeds = []
        for slot, mode, steps in branches:
            e = self.enc(_anchor_ids(queries, slot) if anchors is None else anchors[:, slot].contiguous(), mode)
            for rel, _ in steps:
                e = self.path_dec.project(e, rel)
            embeds.append(e)
        q = self.inter_dec(embeds[0], embeds[1], imode, *embeds[2:])
        for rel, _ in tail:
            q = self.path_dec.project(q, rel)
        return q

    # ------------------------------------------------------------------ reference entry points
    def forward(self, formula, queries, target_nodes, neg_nodes=None, neg_lengths=None):
        plan = self._plan(formula)
        if self._fused_ok(plan):
            scores = self._fused_scores(formula, queries, target_nodes, neg_nodes, neg_lengths, plan)
        else:
            scores = self._composed_scores(formula, queries, target_nodes, neg_nodes, neg_lengths, plan)
        self._check()
        return scores

    # ------------------------------------------------------------------ answering a query (no counterpart in the reference)
    def _chain_candidates(self, plan, n, project):
        """[n, D]: the first n rows of the target mode's table as a chain formula scores them (normalised, then taken
        through the chain's matrices). project(): computes them. In eval() mode the last result is kept (class docstring)."""
        if self.training:
            self.__dict__['_cand'] = None
            return project()
        steps = plan[1][0][2]
        table = self.enc.table(plan[1][0][1])
        path = self.path_dec.vecs if hasattr(self.path_dec, 'vecs') else self.path_dec.mats
        used = [table] + [path[r] for r, _ in steps]
        key = (tuple(r for r, _ in steps), plan[1][0][1], str(table.device), n, bool(self._fused_ok(plan)),
               tuple((t.data_ptr(), t._version) for t in used))
        hit = self.__dict__.get('_cand')
        if hit is None or hit[0] != key:
            hit = self.__dict__['_cand'] = (key, project())
        return hit[1]

    def _rank_operands(self, formula, queries, n, anchors=None):
        """(q [B, D], candidates [n, D], score kind) for ops.rank_entities: that score of (q, candidate) is the one
        forward() gives the pair. anchors: the anchor ids [B, A] on the device in place of `queries` (rank_ids)."""
        plan = self._plan(formula)
        form, branches, imode, tail, emode = plan
        enc, device = self.enc, self._device()
        err = self._error_word(device)
        B = len(queries) if anchors is None else int(anchors.shape[0])
        fused = self._fused_ok(plan)
        if form == 1:
            if fused:
                prog, modes, mats = self._programme(plan)
                if anchors is None:
                    p_ids = np.asarray([_anchor_ids(queries, slot) for slot, _, _ in branches], dtype=np.int64).reshape(-1, B)
                    p_ids = torch.from_numpy(p_ids).to(device)
                else:
                    p_ids = anchors[:, [slot for slot, _, _ in branches]].t().contiguous()
                q = ops.gqe_embed(prog, [enc.table(m) for m in modes], mats, enc.node_maps, p_ids, B, err)
            else:
                q = self._composed_query(queries, plan, anchors).t()
            return q, enc.table(formula.target_mode).detach()[:n], 'cosine'
        steps = branches[0][2]
        table = enc.table(formula.target_mode).detach()

        def project():
            if fused:
                prog, modes, mats = self._programme(plan)
                return ops.gqe_embed(prog, [enc.table(m) for m in modes], mats, None, None, n, err)
            act = ops.embed_l2norm(table, None, torch.arange(n, device=device), err)
            for rel, _ in steps:
                if hasattr(self.path_dec, 'vecs'):
                    act = self.path_dec.project(act.t(), rel).t().detach()
                else:
                    act = ops.linear(act, self.path_dec.mats[rel].detach().t())
            return act.contiguous()
        cand = self._chain_candidates(plan, n, project)
        first = _anchor_ids(queries, 0) if anchors is None else anchors[:, 0].contiguous()
        return enc(first, formula.anchor_modes[0]).t(), cand, self._plan_score(plan)

    def _rank_all(self, formula, queries, target_nodes, exclude, k):
        return self._rank_rows(formula, queries, target_nodes, exclude, k, lambda n: self._rank_operands(formula, queries, n))

    def _rank_operands_ids(self, formula, anchors, n):
        return self._rank_operands(formula, None, n, anchors)

    def _embed_mixed(self, formulas, formula_of, anchors):
        """rank_ids_mixed's query embeddings [B, D] in one ops.gqe_embed_mixed launch, or None: a chain type (its candidates
        are a projected table per formula, which goes by runs) or formulas the fused kernel does not cover"""
        desc, (form, branches, imode, tail, emode) = self._mixed_descriptors(formulas)
        if desc is None or form != 1:
            return None
        p_ids = anchors[:, [slot for slot, _, _ in branches]].t().contiguous()
        return ops.gqe_embed_mixed(desc, self.enc.node_maps, formula_of, p_ids, self._error_word(self._device()))

    def answer(self, formula, queries, k=10, exclude=None):
        """The k entities of formula.target_mode the model proposes for each query, best first:
        (ids [B, k] int64 global entity ids, scores [B, k] float32), -1 / -inf past the last eligible entity. The score is
        the one forward() gives a candidate. `exclude`: one list of entity ids per query that must not be returned.
        Every entity of the mode is scored (mpqe_rank_entities); k <= ops.RANK_MAX_K."""
        if k < 1:
            raise ValueError('answer: k must be at least 1')
        with torch.no_grad():
            ids, scores, _ = self._rank_all(formula, queries, None, exclude, k)
        return ids, scores

    def rank_targets(self, formula, queries, target_nodes=None, exclude=None):
        """ranks [B] int64: 1 + the number of entities of formula.target_mode, other than the target and those in
        `exclude`, that the model places before each query's target (default: query.target_node); ties go to the entity
        with the smaller table row. The target is never excluded, listed or not (the filtered setting passes every known
        answer)."""
        if target_nodes is None:
            target_nodes = [query.target_node for query in queries]
        with torch.no_grad():
            _, _, rank = self._rank_all(formula, queries, target_nodes, exclude, 0)
        return rank

    def sample_negatives(self, formula, queries, hard_negatives=False):
        """reference: model.py:120-127 (same python `random` stream, so the same draws)."""
        return sample_negatives(self.graph, formula, queries, hard_negatives)

    def margin_loss(self, formula, queries, hard_negatives=False, margin=1):
        """reference: model.py:119-134. The reference scores targets and negatives in two forward() calls; here one call
        scores both (neg_lengths of 1), which computes the same numbers."""
        neg_nodes = self.sample_negatives(formula, queries, hard_negatives)
        targets = [query.target_node for query in queries]
        B = len(queries)
        scores = self.forward(formula, queries, targets, neg_nodes=neg_nodes, neg_lengths=[1] * B)
        return ops.hinge(scores[:B], scores[B:], margin)
