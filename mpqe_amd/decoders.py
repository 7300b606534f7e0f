"""The GQE baseline's decoders with the reference's interface (mpqe/decoders.py): the three metapath decoders (bilinear,
TransE, diagonal bilinear) and the two set-intersection operators. Embeddings are columns ([D, B]) at this interface, as in the reference; each forward /
project runs on the library's kernels through ops.linear / ops.cosine / ops.branch_agg. `QueryEncoderDecoder`
(mpqe_amd/model.py) calls them only on its composed path: its fused path reads their parameters and runs one launch.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.init as init

from . import ops


class BilinearMetapathDecoder(nn.Module):
    """reference decoders.py:123-150: one [D, D] matrix per relation triple, a metapath is the product of its matrices."""

    def __init__(self, relations, dims):
        super(BilinearMetapathDecoder, self).__init__()
        self.relations = relations
        self.mats = {}
        for r1 in relations:
            for r2 in relations[r1]:
                rel = (r1, r2[1], r2[0])
                self.mats[rel] = nn.Parameter(torch.FloatTensor(dims[rel[0]], dims[rel[2]]))
                init.xavier_uniform_(self.mats[rel])
                self.register_parameter('_'.join(rel), self.mats[rel])

    def forward(self, embeds1, embeds2, rels):
        """cos(embeds1^T . M[rels[0]] . M[rels[1]] ..., embeds2) per column pair (decoders.py:142-147)."""
        act = embeds1.t()
        for i_rel in rels:
            act = ops.linear(act, self.mats[tuple(i_rel)].t())
        return ops.cosine(act, embeds2.t())

    def project(self, embeds, rel):
        """M[rel] . embeds (decoders.py:149-150)."""
        return ops.linear(embeds.t(), self.mats[tuple(rel)]).t()


class _VectorMetapathDecoder(nn.Module):
    """One [D] vector per relation triple (reference decoders.py:188-197, 217-226: the bilinear decoder's creation order
    and parameter names, uniform(-6 / sqrt(D), 6 / sqrt(D))). forward / project are plain differentiable tensor ops: the
    composed path of `QueryEncoderDecoder`; its fused path reads `vecs`, `op` and `score` and runs one launch."""
    op = None           # ops.gqe_programme's path operator
    score = None        # how forward() scores a chain: 'cosine' | 'dot'

    def __init__(self, relations, dims):
        super(_VectorMetapathDecoder, self).__init__()
        self.relations = relations
        self.vecs = {}
        for r1 in relations:
            for r2 in relations[r1]:
                rel = (r1, r2[1], r2[0])
                self.vecs[rel] = nn.Parameter(torch.FloatTensor(dims[rel[0]]))
                bound = 6.0 / np.sqrt(dims[rel[0]])
                init.uniform_(self.vecs[rel], a=-bound, b=bound)
                self.register_parameter('_'.join(rel), self.vecs[rel])


class TransEMetapathDecoder(_VectorMetapathDecoder):
    """reference decoders.py:181-208: a relation translates, a metapath adds its vectors one after another."""
    op, score = 'translate', 'cosine'

    def forward(self, embeds1, embeds2, rels):
        """cos(embeds2, ((embeds1 + v[rels[0]]) + v[rels[1]]) ...) per column pair (decoders.py:200-205; the reference adds
        in place into embeds1, which changes no value)."""
        act = embeds1
        for i_rel in rels:
            act = act + self.vecs[tuple(i_rel)].unsqueeze(1)
        return nn.functional.cosine_similarity(embeds2, act, dim=0)

    def project(self, embeds, rel):
        return embeds + self.vecs[tuple(rel)].unsqueeze(1)


class BilinearDiagMetapathDecoder(_VectorMetapathDecoder):
    """reference decoders.py:211-236: a relation scales, and a chain is scored by the plain dot product (no cosine)."""
    op, score = 'scale', 'dot'

    def forward(self, embeds1, embeds2, rels):
        act = embeds1
        for i_rel in rels:
            act = act * self.vecs[tuple(i_rel)].unsqueeze(1)
        return (act * embeds2).sum(0)

    def project(self, embeds, rel):
        return embeds * self.vecs[tuple(rel)].unsqueeze(1)


def _agg_kind(agg_func):
    if agg_func is torch.min:
        return 'min'
    if agg_func is torch.mean:
        return 'mean'
    raise NotImplementedError('set intersection: agg_func must be torch.min or torch.mean (the reference\'s two options)')


class SetIntersection(nn.Module):
    """reference decoders.py:270-300: post[mode] . agg_k(relu(pre[mode] . e_k)) over two or three branches."""

    def __init__(self, mode_dims, expand_dims, agg_func=torch.min):
        super(SetIntersection, self).__init__()
        self.pre_mats = {}
        self.post_mats = {}
        self.agg_func = agg_func
        self.agg_kind = _agg_kind(agg_func)
        for mode in mode_dims:
            self.pre_mats[mode] = nn.Parameter(torch.FloatTensor(expand_dims[mode], mode_dims[mode]))
            init.xavier_uniform_(self.pre_mats[mode])
            self.register_parameter(mode + '_premat', self.pre_mats[mode])
            self.post_mats[mode] = nn.Parameter(torch.FloatTensor(mode_dims[mode], expand_dims[mode]))
            init.xavier_uniform_(self.post_mats[mode])
            self.register_parameter(mode + '_postmat', self.post_mats[mode])

    def forward(self, embeds1, embeds2, mode, embeds3=[]):
        branches = [embeds1, embeds2] + ([embeds3] if len(embeds3) > 0 else [])
        hidden = [ops.linear(e.t(), self.pre_mats[mode], relu=True) for e in branches]
        combined = ops.branch_agg(hidden, self.agg_kind)
        return ops.linear(combined, self.post_mats[mode]).t()


class SimpleSetIntersection(nn.Module):
    """reference decoders.py:302-319: the element-wise mean / min of the branches."""

    def __init__(self, agg_func=torch.min):
        super(SimpleSetIntersection, self).__init__()
        self.agg_func = agg_func
        self.agg_kind = _agg_kind(agg_func)

    def forward(self, embeds1, embeds2, mode, embeds3=[]):
        branches = [embeds1, embeds2] + ([embeds3] if len(embeds3) > 0 else [])
        return ops.branch_agg([e.t() for e in branches], self.agg_kind).t()
