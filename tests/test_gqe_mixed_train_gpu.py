"""QueryEncoderDecoder.margin_loss_ids_mixed (one mpqe_gqe_fwd_mixed_save + one mpqe_gqe_bwd_mixed per window) against
margin_loss_ids_by_runs (the per-formula route: ops.gqe_scores run by run), kg.MixedQuerySet.take / negative_sampler and
tools/train_synthetic.py --mixed-train. Built like tests/test_eval_mixed_sets.py: the `tiny` graph of
tests/test_kg_sample.py, sample_query_sets(batched=True), D 32.

Tolerances: the loss within FWD and every parameter's .grad within TWO times BWD of tests/gqe_oracle.py -- both routes
are within BWD of the truth, and their states are bit-identical (the mixed kernels' rows are the per-formula kernels'
rows), so no discrete choice -- a minimum, a ReLU -- can differ between them."""
import copy

import numpy as np
import pytest
import torch

from mpqe_amd.kg import MixedQuerySet
from mpqe_amd.model import margin_loss_ids_by_runs
from tests.gqe_oracle import BWD, FWD
from tests.test_eval_sets import NEG_MAX, TYPES
from tests.test_kg_sample import tiny               # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
WINDOW = 64


def _model(tiny, D, inter='mean', seed=11):
    from mpqe_amd import synthetic
    from mpqe_amd.data_utils import make_feature_modules
    from mpqe_amd.encoders import DirectEncoder
    from mpqe_amd.model import QueryEncoderDecoder
    from mpqe_amd.utils import get_intersection_decoder, get_metapath_decoder
    schema, adj, _, _ = tiny
    torch.manual_seed(seed)
    graph = synthetic.SchemaGraph(schema, D)
    graph.adj_lists = adj
    fm, node_maps = make_feature_modules(schema.ids, D, schema.num_entities)
    dims = {m: D for m in schema.modes}
    model = QueryEncoderDecoder(graph, DirectEncoder(None, fm, node_maps), get_metapath_decoder(graph, dims, 'bilinear'),
                                get_intersection_decoder(graph, dims, inter))
    return graph, node_maps, model.to('cuda:0')


@pytest.fixture(scope='module')
def world(tiny):
    """the model (D 32), the mixed training sets of all seven types and one window of 64 positions a type with its negatives"""
    from mpqe_amd.kg import KGIndex
    graph, node_maps, model = _model(tiny, 32)
    index = KGIndex.from_graph(graph, node_maps, torch.device('cuda:0'))
    sets = index.sample_query_sets(TYPES, 96, seed=3, neg_sample_max=NEG_MAX, batched=True)
    mixed = MixedQuerySet.from_sets(sets)
    assert set(mixed) == set(TYPES)
    gen = torch.Generator().manual_seed(5)
    windows = {}
    for k, (qt, ms) in enumerate(mixed.items()):
        idx = torch.sort(torch.randint(len(ms), (WINDOW,), generator=gen, dtype=torch.long)).values.cuda()
        sampler = ms.negative_sampler()
        neg = sampler.sample(idx, 100 + k, hard_negatives='inter' in qt)
        sampler.check()
        windows[qt] = ms.take(idx) + (neg,)
    return tiny, model, mixed, windows


def _loss_and_grads(model, fn):
    model.zero_grad(set_to_none=True)
    loss = fn()
    loss.backward()
    grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.named_parameters()}
    model.zero_grad(set_to_none=True)
    return loss.detach().clone(), grads


def _assert_close(loss, grads, want_loss, want_grads):
    np.testing.assert_allclose(loss.cpu().numpy(), want_loss.cpu().numpy(), **FWD)
    some = 0
    for k, w in want_grads.items():
        g = grads[k]
        if w is None:                    # (the mixed route hands zeros to a parameter no query of the window names)
            assert g is None or not g.any(), k
            continue
        assert g is not None, k
        some += bool(w.any())
        np.testing.assert_allclose(g.cpu().numpy(), w.cpu().numpy(), rtol=2 * BWD['rtol'], atol=2 * BWD['atol'], err_msg=k)
    assert some >= 2


@pytest.mark.parametrize('qt', TYPES)
def test_loss_and_gradients_against_the_walk_over_runs(world, qt):
    _, model, mixed, windows = world
    ms = mixed[qt]
    fo, anchors, targets, neg = windows[qt]
    assert len(set(fo.tolist())) > 1 and fo.shape[0] == WINDOW                  # (something is mixed)
    got = _loss_and_grads(model, lambda: model.margin_loss_ids_mixed(ms.formulas, fo, anchors, targets, neg))
    assert model.__dict__['_mixed'][id(ms.formulas)][2] is not None             # (the mixed launch, not the fallback)
    want = _loss_and_grads(model, lambda: margin_loss_ids_by_runs(model, ms.formulas, fo, anchors, targets, neg))
    _assert_close(got[0], got[1], want[0], want[1])
    # two calls from equal models: the same bits
    twin = copy.deepcopy(model)
    again = _loss_and_grads(twin, lambda: twin.margin_loss_ids_mixed(ms.formulas, fo, anchors, targets, neg))
    assert torch.equal(got[0], again[0])
    for k, g in got[1].items():
        assert (g is None) == (again[1][k] is None) and (g is None or torch.equal(g, again[1][k])), k


def test_take_and_sampler(world):
    _, model, mixed, windows = world
    ms = mixed['2-inter']
    idx = torch.tensor([5, 0, 5, len(ms) - 1], dtype=torch.long, device='cuda:0')
    fo, anchors, targets = ms.take(idx)
    assert torch.equal(fo, ms.formula_of[idx]) and torch.equal(anchors, ms.anchors[idx]) and torch.equal(targets, ms.targets[idx])
    with pytest.raises(TypeError):
        ms.take([0, 1])
    sampler = mixed['1-chain'].negative_sampler()
    one = mixed['1-chain']
    idx = torch.arange(len(one), dtype=torch.long, device='cuda:0')
    neg = sampler.sample(idx, 7).cpu().numpy()
    ids, off = (t.cpu().numpy() for t in one.neg)
    # (a mixed 1-chain window draws from each query's sampled negatives, not from the whole target mode)
    assert all(neg[i] in ids[off[i]:off[i + 1]] for i in range(len(one)))


@pytest.mark.parametrize('why', ['not fused', 'D 24'])
def test_fallbacks_take_the_walk_over_runs(world, why, monkeypatch):
    """No descriptor block (fused = False; a D the kernel does not take): margin_loss_ids_mixed IS one call of
    margin_loss_ids_by_runs -- watched here -- and gives its numbers. The composed ops' table gradient is not the same
    bits from one call to the next, so a second call of the walk is compared as the two routes are above, not bit for bit."""
    from mpqe_amd import model as model_module
    tiny_, model, mixed, windows = world
    if why == 'D 24':
        _, _, model = _model(tiny_, 24)
    else:
        model = copy.deepcopy(model)
        model.fused = False
    ms = mixed['3-inter_chain']
    fo, anchors, targets, neg = windows['3-inter_chain']
    calls = []
    real = model_module.margin_loss_ids_by_runs

    def spy(*args, **kwargs):
        calls.append(args[0])
        return real(*args, **kwargs)
    monkeypatch.setattr(model_module, 'margin_loss_ids_by_runs', spy)
    got = _loss_and_grads(model, lambda: model.margin_loss_ids_mixed(ms.formulas, fo, anchors, targets, neg))
    assert calls == [model] and model.__dict__['_mixed'][id(ms.formulas)][2] is None
    want = _loss_and_grads(model, lambda: real(model, ms.formulas, fo, anchors, targets, neg))
    assert torch.equal(got[0], want[0])
    _assert_close(got[0], got[1], want[0], want[1])
    assert all((w is None) == (got[1][k] is None) for k, w in want[1].items())


def test_the_kept_block_follows_the_addresses(world):
    _, model, mixed, windows = world
    model = copy.deepcopy(model)
    ms = mixed['2-chain']
    fo, anchors, targets, neg = windows['2-chain']

    def step():
        loss = model.margin_loss_ids_mixed(ms.formulas, fo, anchors, targets, neg)
        loss.backward()
        return model.__dict__['_mixed'][id(ms.formulas)][2]
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    first = step()
    opt.step()
    assert step() is first                                  # an optimizer step keeps the block
    model.to('cpu')
    model.to('cuda:0')
    moved = step()
    assert moved is not first                               # the parameters moved: rebuilt
    rel = tuple(ms.formulas[0].rels[0])
    fresh = torch.nn.Parameter(model.path_dec.mats[rel].detach().clone())
    model.path_dec.mats[rel] = fresh
    model.path_dec.register_parameter('_'.join(rel), fresh)
    assert step() is not moved                              # a parameter replaced: rebuilt
    # the op itself refuses tensors the block was not built on
    from mpqe_amd import ops
    desc = model.__dict__['_mixed'][id(ms.formulas)][2]
    tables = [t.detach().clone().requires_grad_(True) for t in desc.live[0]]
    with pytest.raises(ValueError):
        ops.gqe_scores_mixed_grad(desc, tables, desc.live[1], model.enc.node_maps, fo, torch.cat([targets, neg]).reshape(1, -1),
                                  anchors[:, 0].contiguous(), torch.arange(WINDOW, device='cuda:0').repeat(2), None, 2 * WINDOW)


def test_formulas_of_two_query_types_are_refused(world):
    _, model, mixed, windows = world
    fo, anchors, targets, neg = windows['2-chain']
    both = mixed['2-chain'].formulas[:1] + mixed['3-chain'].formulas[:1]
    with pytest.raises(ValueError):
        model.margin_loss_ids_mixed(both, fo, anchors, targets, neg)


def test_mixed_train_tool_is_reproducible_and_learns():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import train_synthetic
    argv = ['--model', 'gqe', '--kg', 'small', '--embed-dim', '32', '--steps', '40', '--device-queries', '--batched-queries',
            '--mixed-train', '--train-queries', '64', '--test-queries', '32']
    runs = [train_synthetic.main(argv) for _ in range(2)]
    curve = np.array(runs[0]['loss_curve'], dtype=np.float64)
    assert runs[0]['mixed_train'] is True and curve.shape == (40,)
    assert curve.tobytes() == np.array(runs[1]['loss_curve'], dtype=np.float64).tobytes()
    assert np.isfinite(curve).all()
    assert curve[-10:].mean() < curve[0]
    with pytest.raises(SystemExit):
        train_synthetic.main(['--model', 'gqe', '--mixed-train'])
