"""The neighbourhood-aggregating Encoder on the device KG index (mpqe_amd/encoders.py with index=, utils.get_encoder,
KGIndex.sample_neighbours, ops.sage_encode) on the GPU: forward and every parameter gradient against the float64 oracle of
tests/sage_oracle.py fed the samples the call itself made (enc.last_sample), layer by layer at depth 2; repeatability;
agreement with the host path where both take whole neighbourhoods; state_dict; the fall-back for a shape the fused kernel
does not cover; and both models on such an encoder.

Tolerances: `close` of tests/test_op_edges.py (forward rtol 1e-5, gradients rtol 1e-4, atol 2e-6 x max(1, max |ref|))."""
import json
import os
import random
from collections import OrderedDict

import numpy as np
import pytest
import torch

from mpqe_amd import synthetic
from mpqe_amd.data_utils import make_feature_modules
from mpqe_amd.encoders import DirectEncoder, Encoder
from mpqe_amd.graph import reverse_relation
from mpqe_amd.kg import KGIndex
from mpqe_amd.utils import get_encoder, get_intersection_decoder, get_metapath_decoder
from tests import sage_oracle as oracle
from tests.test_op_edges import close

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
B = 40


def _f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _world(D, seed=5, every_node_has_a_neighbour=False):
    """the `tiny` synthetic KG (60 entities, 3 modes) with a real adjacency -> (graph, feature modules, node_maps, index)"""
    schema = synthetic.make_schema(*synthetic.KG_SHAPES['tiny'], seed=seed)
    adj = synthetic.make_adjacency(schema, degree=3, seed=seed)
    if every_node_has_a_neighbour:
        fix = np.random.RandomState(seed + 101)
        for rel in list(adj):
            for n, nb in adj[rel].items():
                if len(nb) == 0:
                    d = int(fix.choice(schema.ids[rel[2]]))
                    nb.add(d)
                    adj[reverse_relation(rel)][d].add(n)
    else:
        assert any(len(nb) == 0 for lists in adj.values() for nb in lists.values())     # the padding row is exercised
    torch.manual_seed(seed)
    fm, node_maps = make_feature_modules(schema.ids, D, schema.num_entities)
    graph = synthetic.SchemaGraph(schema, D)
    graph.adj_lists = adj
    node_maps = node_maps.to(DEV)
    graph.features = lambda nodes, mode: fm[mode](node_maps[torch.as_tensor(nodes, dtype=torch.long, device=DEV)])
    return graph, fm, node_maps, KGIndex.from_graph(graph, node_maps, DEV)


def _nodes(graph, mode, seed=1):
    rng = np.random.RandomState(seed)
    return [int(x) for x in rng.choice(graph.schema.ids[mode], size=B, replace=True)]


def _spread(enc, factor=4.0):
    """larger compress matrices and non-trivial gamma / beta: outputs of the scale of their inputs"""
    with torch.no_grad():
        for name, p in enc.named_parameters():
            if name.endswith('_compress'):
                p.mul_(factor)
            elif name.endswith('gamma'):
                p.add_(0.3 * torch.randn_like(p))
            elif name.endswith('beta'):
                p.add_(0.3 * torch.randn_like(p))


class _Oracle(object):
    """The float64 oracle applied to one recorded call, recursively over the inner encoders' calls (depth >= 2)."""

    def __init__(self, enc, sample):
        self.enc, mode = enc, sample['mode']
        rels, rows = sample['relations'], sample['rows'].cpu().numpy()
        R, n = len(rels), rows.shape[0]
        self.W = enc.compress_params[mode]
        self.ln = enc.lns[mode] if enc.layer_norm else None
        counts = sample['counts'].cpu().numpy()
        if sample['inner'] is None:
            self.children, modes = None, []
            for m in [r[2] for r in rels] + [mode]:
                if m not in modes:
                    modes.append(m)
            self.leaves = [enc.feature_modules[m].weight for m in modes]
            tables = [_f64(t) for t in self.leaves]
            block_table = [modes.index(r[2]) for r in rels] + [modes.index(mode)]
            neigh, self_rows = sample['neigh'].cpu().numpy(), rows
        else:
            models = {'base': enc.base_model, 'self': enc._self_model[0]}
            self.children = [_Oracle(models[rec['encoder']], rec['sample']) for rec in sample['inner']]
            tables = [c.out for c in self.children]
            where, mk = sample['where'], sample['max_keep']
            block_table = [g for g, _ in where]
            slots = np.arange(n * mk, dtype=np.int64).reshape(n, mk)
            neigh = np.stack([slots + first for _, first in where[:-1]])
            self_rows = np.arange(n, dtype=np.int64) + where[-1][1]
        pad = [tables[t].shape[0] - 1 for t in block_table]
        gamma = None if self.ln is None else _f64(self.ln.gamma)
        beta = None if self.ln is None else _f64(self.ln.beta)
        self.args = (tables, block_table, pad, neigh, counts, self_rows, _f64(self.W))
        self.kw = dict(gamma=gamma, beta=beta, eps=float(np.float32(1e-6)))
        self.st = oracle.forward(*self.args, **self.kw)
        self.out = self.st['out']

    def backward(self, grad_out, acc):
        """adds every parameter's gradient to acc {id(parameter): float64 array}"""
        g_tables, g_W, g_gamma, g_beta = oracle.backward(*self.args, grad_out, st=self.st, **self.kw)

        def add(p, g):
            acc[id(p)] = acc.get(id(p), 0.0) + g
        add(self.W, g_W)
        if self.ln is not None:
            add(self.ln.gamma, g_gamma)
            add(self.ln.beta, g_beta)
        for k, g in enumerate(g_tables):
            if self.children is None:
                add(self.leaves[k], g)
            else:
                self.children[k].backward(g, acc)


def _against_the_oracle(enc, graph, mode, keep_prob=0.5, max_keep=10, what=''):
    nodes = _nodes(graph, mode)
    nodes[3] = -1                                           # a null node in the batch
    random.seed(7)
    out = enc(torch.tensor(nodes, dtype=torch.int64), mode, keep_prob=keep_prob, max_keep=max_keep)
    assert tuple(out.shape) == (enc.out_dims[mode], B)
    gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    out.backward(gout)
    ref = _Oracle(enc, enc.last_sample)
    close(out.detach().cpu().numpy().T, ref.out, what=what + ' out')
    acc = {}
    ref.backward(_f64(gout).T, acc)
    for name, p in enc.named_parameters():
        want = acc.get(id(p))
        got = np.zeros(tuple(p.shape)) if p.grad is None else _f64(p.grad)
        close(got, np.zeros(tuple(p.shape)) if want is None else want, rtol=1e-4, what='%s grad %s' % (what, name))
    assert int(enc._err.item()) == 0
    counts = enc.last_sample['counts'].cpu().numpy()
    assert (counts == 0).any() and (counts > 1).any()
    return out


# ---------------------------------------------------------------------------------------------- depth 1 and 2
@pytest.mark.parametrize('layer_norm', [False, True])
@pytest.mark.parametrize('D', [16, 64])
def test_depth_1_against_the_oracle(D, layer_norm):
    graph, fm, node_maps, index = _world(D)
    dims = {m: D for m in graph.schema.modes}
    from mpqe_amd.aggregators import MeanAggregator
    enc = Encoder(graph.features, dims, dims, graph.relations, graph.adj_lists, MeanAggregator(graph.features), cuda=True,
                  layer_norm=layer_norm, feature_modules=fm, index=index, node_maps=node_maps).to(DEV)
    _spread(enc)
    for mode in graph.schema.modes[:2]:
        enc.zero_grad()
        _against_the_oracle(enc, graph, mode, what='depth 1, D %d, %s' % (D, mode))


@pytest.mark.parametrize('D', [16, 64])
def test_depth_2_against_the_oracle_layer_by_layer(D):
    graph, fm, node_maps, index = _world(D)
    dims = {m: D for m in graph.schema.modes}
    enc = get_encoder(2, graph, dims, fm, True, node_maps=node_maps, index=index).to(DEV)
    _spread(enc)
    mode = graph.schema.modes[0]
    _against_the_oracle(enc, graph, mode, what='depth 2, D %d' % D)
    inner = enc.last_sample['inner']
    assert len(inner) == len({(r['encoder'], r['mode']) for r in inner})            # one inner call per destination mode
    assert all(r['sample']['keep_prob'] == 0.5 and r['sample']['max_keep'] == 10 for r in inner)      # the defaults


def test_depth_3_takes_its_own_features_from_the_first_encoder():
    graph, fm, node_maps, index = _world(16)
    dims = {m: 16 for m in graph.schema.modes}
    enc = get_encoder(3, graph, dims, fm, True, node_maps=node_maps, index=index).to(DEV)
    assert enc._self_model[0] is enc.base_model.base_model and enc.base_model._self_model[0] is enc.base_model.base_model
    _spread(enc)
    nodes = _nodes(graph, graph.schema.modes[0])[:6]
    random.seed(1)
    out = enc(nodes, graph.schema.modes[0], keep_prob=0.5, max_keep=2)
    ref = _Oracle(enc, enc.last_sample)
    close(out.detach().cpu().numpy().T, ref.out, what='depth 3 out')
    assert {r['encoder'] for r in enc.last_sample['inner']} == {'base', 'self'}


# ---------------------------------------------------------------------------------------------- repeatability, host path
def test_same_seed_same_bits_and_agreement_with_the_host_path():
    D = 16
    graph, fm, node_maps, index = _world(D, every_node_has_a_neighbour=True)
    dims = {m: D for m in graph.schema.modes}
    dev_enc = get_encoder(1, graph, dims, fm, True, node_maps=node_maps, index=index).to(DEV)
    host_enc = get_encoder(1, graph, dims, fm, True, node_maps=node_maps).to(DEV)
    host_enc.load_state_dict(dev_enc.state_dict(), strict=True)
    assert list(dev_enc.state_dict()) == list(host_enc.state_dict())
    mode = graph.schema.modes[1]
    nodes = _nodes(graph, mode)
    runs = []
    for _ in range(2):
        random.seed(11)
        dev_enc.zero_grad()
        out = dev_enc(nodes, mode)
        out.sum().backward()
        runs.append([out.detach().clone()] + [p.grad.clone() for _, p in sorted(dev_enc.named_parameters()) if p.grad is not None])
    assert len(runs[0]) == len(runs[1]) and all(torch.equal(a, b) for a, b in zip(*runs))
    random.seed(12)
    assert not torch.equal(dev_enc(nodes, mode), runs[0][0])                        # another seed, other draws
    # whole neighbourhoods on both paths, whatever the stream
    degree = max(len(nb) for lists in graph.adj_lists.values() for nb in lists.values())
    assert 1 < degree <= 32
    gout = torch.randn((D, B), generator=torch.Generator().manual_seed(4)).to(DEV)
    got = {}
    for name, enc in (('device', dev_enc), ('host', host_enc)):
        enc.zero_grad()
        out = enc(nodes, mode, keep_prob=1.0, max_keep=32)
        out.backward(gout)
        got[name] = (out.detach().cpu().numpy(), {k: _f64(p.grad) for k, p in enc.named_parameters() if p.grad is not None})
    close(got['device'][0], got['host'][0], what='device path against host path, out')
    assert set(got['device'][1]) == set(got['host'][1])
    for k, g in got['host'][1].items():
        close(got['device'][1][k], g, rtol=1e-4, what='device path against host path, grad ' + k)


# ---------------------------------------------------------------------------------------------- state, fall-back
@pytest.mark.parametrize('name', ['sage_depth1_plain', 'sage_depth1_ln'])
def test_state_dict_keys_and_strict_load_of_the_reference_parameters(name):
    from mpqe_amd.aggregators import MeanAggregator
    z = np.load(os.path.join(GOLDEN, name + '.npz'))
    meta = json.loads(bytes(z['meta']).decode())
    D, modes = meta['D'], meta['schema']['modes']
    relations = OrderedDict((m, [tuple(x) for x in meta['schema']['relations'][m]]) for m in modes)
    adj = {tuple(rel): {int(n): list(nb) for n, nb in items} for rel, items in meta['adj']}
    ids = {m: meta['schema']['ids'][m] for m in modes}
    edges = {rel: (np.repeat(list(lists), [len(v) for v in lists.values()]), np.array([x for v in lists.values() for x in v]))
             for rel, lists in adj.items()}
    index = KGIndex.from_edges(ids, edges, z['node_map'], DEV)
    fm = {m: torch.nn.Embedding(len(ids[m]) + 1, D) for m in modes}
    dims = {m: D for m in modes}
    enc = Encoder(None, dims, dims, relations, None, None, cuda=True, layer_norm=meta['layer_norm'], feature_modules=fm,
                  index=index)
    state = {k[len('param/'):]: torch.from_numpy(z[k]) for k in z.files if k.startswith('param/')}
    assert set(enc.state_dict()) == set(state)
    enc.load_state_dict(state, strict=True)
    enc = enc.to(DEV)
    # whole neighbourhoods: the draws do not matter, so the reference's own output is not reproduced here (its max_keep
    # of 2 cuts lists); the loaded parameters give a finite output of the reference's shape
    out = enc(z['nodes'].tolist(), meta['mode'], keep_prob=meta['keep_prob'], max_keep=meta['max_keep'])
    assert tuple(out.shape) == tuple(z['out'].shape) and torch.isfinite(out).all()
    assert int(enc._err.item()) == 0


def test_an_unsupported_width_falls_back_and_agrees_with_the_oracle():
    D = 24
    graph, fm, node_maps, index = _world(D)
    dims = {m: D for m in graph.schema.modes}
    enc = get_encoder(1, graph, dims, fm, True, node_maps=node_maps, index=index).to(DEV)
    _spread(enc)
    _against_the_oracle(enc, graph, graph.schema.modes[0], what='D 24 (per-op kernels)')


# ---------------------------------------------------------------------------------------------- the models
@pytest.mark.parametrize('model_name', ['gqe', 'rgcn'])
def test_models_train_through_the_device_encoder(model_name):
    from mpqe_amd.model import QueryEncoderDecoder, RGCNEncoderDecoder
    D = 16
    graph, fm, node_maps, index = _world(D)
    dims = {m: D for m in graph.schema.modes}
    enc = get_encoder(1, graph, dims, fm, True, node_maps=node_maps, index=index)
    if model_name == 'gqe':
        model = QueryEncoderDecoder(graph, enc, get_metapath_decoder(graph, dims, 'bilinear'),
                                    get_intersection_decoder(graph, dims, 'mean'))
    else:
        model = RGCNEncoderDecoder(graph, enc, readout='mp', num_layers=2, weight_decay=0)
    model = model.to(DEV)
    rng = np.random.RandomState(2)
    random.seed(5)
    for qt in ('1-chain', '2-inter'):
        formula = synthetic.sample_formula(graph.schema, qt, rng)
        queries = synthetic.sample_queries(graph.schema, formula, 24, rng)
        model.zero_grad()
        loss = model.margin_loss(formula, queries)
        assert torch.isfinite(loss).all()
        loss.backward()
        compress = [p for n, p in enc.named_parameters() if n.endswith('_compress') and p.grad is not None]
        assert compress and any(float(p.grad.abs().max()) > 0 for p in compress)
        tables = [m.weight for m in fm.values() if m.weight.grad is not None]
        assert tables and any(float(t.grad.abs().max()) > 0 for t in tables)
        assert int(enc._err.item()) == 0 and (model._err is None or int(model._err.item()) == 0)
