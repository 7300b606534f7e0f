"""RGCNEncoderDecoder.margin_loss_ids_mixed (one mpqe_rgcn_fwd_mixed_save + one mpqe_rgcn_bwd_mixed per window) against
margin_loss_ids_by_runs (the module path run by run) on the same model. Built like tests/test_rgcn_mixed_sets.py: the
`tiny` graph, all seven query types, several formulas a type, three distinct layers, adaptive passes.

Tolerances: the loss within FWD and every parameter's .grad within BWD of tests/gqe_oracle.py. The two routes' states are
bit-identical (the mixed forward's rows are the module path's rows), so no discrete choice -- a ReLU, a maximum -- can
differ between them; what differs is the order of the sums into a parameter's gradient."""
import copy

import numpy as np
import pytest
import torch

from mpqe_amd import model as model_module
from mpqe_amd import ops
from mpqe_amd.model import margin_loss_ids_by_runs
from tests.gqe_oracle import BWD, FWD
from tests.test_eval_sets import TYPES
from tests.test_kg_sample import tiny               # noqa: F401  (the fixture)
from tests.test_rgcn_mixed_sets import build

pytestmark = pytest.mark.gpu


def window(mixed, qt, seed=100):
    """every query of the type's mixed set with one drawn negative each"""
    ms = mixed[qt]
    idx = torch.arange(len(ms), dtype=torch.long, device='cuda:0')
    sampler = ms.negative_sampler()
    neg = sampler.sample(idx, seed, hard_negatives='inter' in qt)
    sampler.check()
    return ms, ms.take(idx) + (neg,)


def loss_and_grads(model, fn):
    model.zero_grad(set_to_none=True)
    loss = fn()
    loss.backward()
    grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.named_parameters()}
    model.zero_grad(set_to_none=True)
    return loss.detach().clone(), grads


def assert_close(got, want):
    np.testing.assert_allclose(got[0].cpu().numpy(), want[0].cpu().numpy(), **FWD)
    some = 0
    for k, w in want[1].items():
        g = got[1][k]
        if w is None:                    # (the mixed route hands zeros to a parameter no query of the window names)
            assert g is None or not g.any(), k
            continue
        assert g is not None, k
        some += bool(w.any())
        print('%s: max abs difference %.3g (max |walk| %.3g)' % (k, float((g - w).abs().max()), float(w.abs().max())))
        np.testing.assert_allclose(g.cpu().numpy(), w.cpu().numpy(), err_msg=k, **BWD)
    assert some >= 3


class Spy(object):
    """calls of a module-level function of mpqe_amd.model or mpqe_amd.ops, counted"""

    def __init__(self, monkeypatch, module, name):
        self.n, real = 0, getattr(module, name)

        def spy(*args, **kwargs):
            self.n += 1
            return real(*args, **kwargs)
        monkeypatch.setattr(module, name, spy)


@pytest.mark.parametrize('readout', ['mp', 'sum', 'max'])
@pytest.mark.parametrize('qt', TYPES)
def test_loss_and_gradients_against_the_walk_over_runs(tiny, monkeypatch, qt, readout):  # noqa: F811
    index, sets, mixed, model = build(tiny, 16, readout)
    ms, (fo, anchors, targets, neg) = window(mixed, qt)
    assert len(set(fo.tolist())) > 1                                            # (something is mixed)
    mixed_calls, walks = Spy(monkeypatch, ops, 'rgcn_scores_mixed_grad'), Spy(monkeypatch, model_module, 'margin_loss_ids_by_runs')
    got = loss_and_grads(model, lambda: model.margin_loss_ids_mixed(ms.formulas, fo, anchors, targets, neg))
    assert (mixed_calls.n, walks.n) == (1, 0)                                   # (the mixed launch, not the fallback)
    want = loss_and_grads(model, lambda: margin_loss_ids_by_runs(model, ms.formulas, fo, anchors, targets, neg))
    assert_close(got, want)
    assert model._err is None or int(model._err.item()) == 0
    # a second call: the same bits
    again = loss_and_grads(model, lambda: model.margin_loss_ids_mixed(ms.formulas, fo, anchors, targets, neg))
    assert torch.equal(got[0], again[0])
    for k, g in got[1].items():
        h = again[1][k]
        if g is None or h is None:       # (a parameter outside the window's passes: no gradient, or zeros once a step owns it)
            assert (g is None or not g.any()) and (h is None or not h.any()), k
        else:
            assert torch.equal(g, h), k


def test_wider_rows(tiny):  # noqa: F811
    index, sets, mixed, model = build(tiny, 128, 'mp')
    ms, (fo, anchors, targets, neg) = window(mixed, '3-inter_chain')
    got = loss_and_grads(model, lambda: model.margin_loss_ids_mixed(ms.formulas, fo, anchors, targets, neg))
    want = loss_and_grads(model, lambda: margin_loss_ids_by_runs(model, ms.formulas, fo, anchors, targets, neg))
    assert_close(got, want)


def test_the_kept_blocks_are_reused_and_follow_the_addresses(tiny):  # noqa: F811
    index, sets, mixed, model = build(tiny)
    model = copy.deepcopy(model)
    ms, (fo, anchors, targets, neg) = window(mixed, '2-chain')

    def step():
        model.margin_loss_ids_mixed(ms.formulas, fo, anchors, targets, neg).backward()
        return model.__dict__['_mixed'][id(ms.formulas)][2]
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    first = step()
    assert first is not None and first.index_ptr % 256 == 0
    opt.step()
    assert step() is first                                  # an optimizer step keeps the blocks
    # (scoring finds the same entry)
    model.score_ids_mixed(ms.formulas, fo, anchors, targets)
    assert model.__dict__['_mixed'][id(ms.formulas)][2] is first
    model.to('cpu')
    model.to('cuda:0')
    assert step() is not first                              # the parameters moved: rebuilt
    # the op itself refuses tables the block was not built on
    desc = model.__dict__['_mixed'][id(ms.formulas)][2]
    tables = [t.detach().clone().requires_grad_(True) for t in desc.live]
    layers = [(l.basis, l.root, l.bias) for l in model.layers]
    with pytest.raises(ValueError):
        ops.rgcn_scores_mixed_grad(desc, tables, model.mode_embeddings.weight, layers[-1:], [0, 0], model.enc.node_maps, 'mp', fo,
                                   anchors, torch.cat([targets, neg]), torch.arange(len(ms) + 1, device='cuda:0'))


def test_an_adam_step_changes_the_touched_rows_and_layers_only(tiny):  # noqa: F811
    index, sets, mixed, model = build(tiny)
    model = copy.deepcopy(model)
    ms, (fo, anchors, targets, neg) = window(mixed, '1-chain')          # (adaptive: one pass, the LAST layer alone)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    opt.zero_grad()
    model.margin_loss_ids_mixed(ms.formulas, fo, anchors, targets, neg).backward()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    opt.step()
    changed_any = 0
    for k, p in model.named_parameters():
        moved = (p.detach() != before[k])
        if k not in grads:
            assert not moved.any(), k
            continue
        assert torch.equal(moved, grads[k] != 0), k         # (Adam moves exactly the elements with a gradient)
        changed_any += bool(moved.any())
    last = len(model.layers) - 1
    for k in grads:
        if k.startswith('layers.') and not k.startswith('layers.%d.' % last):
            assert not grads[k].any(), k                    # (zeros, not None: the window names no pass of that layer)
    assert grads['layers.%d.root' % last].any() and grads['layers.%d.basis' % last].any()
    assert changed_any >= 4
    # the tables: rows of entities that are neither anchor, target nor negative have no gradient
    tabs = [k for k in grads if 'enc' in k and grads[k].dim() == 2 and grads[k].any()]
    assert tabs and all((grads[k] == 0).all(dim=1).any() for k in tabs)


def test_a_bad_id_sets_the_error_word_and_the_guarded_step_is_refused(tiny):  # noqa: F811
    from mpqe_amd import optim
    index, sets, mixed, model = build(tiny)
    model = copy.deepcopy(model)
    ms, (fo, anchors, targets, neg) = window(mixed, '2-inter')
    opt = optim.Adam([p for p in model.parameters() if p.requires_grad], lr=0.01)
    assert opt.flat and opt._impl.guard
    opt.zero_grad()
    model.margin_loss_ids_mixed(ms.formulas, fo, anchors, targets, neg).backward()
    start = {k: p.detach().clone() for k, p in model.named_parameters()}
    opt.step()                                              # (a clean step goes through)
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    assert sum(not torch.equal(before[k], start[k]) for k in start) >= 4
    word = model.dropin().step.err                          # (the word the flat update's guard reads)
    bad = targets.clone()
    bad[3] = 10 ** 9
    model.validate = False                                  # (the unchecked loop: nobody reads the word before the step)
    opt.zero_grad()
    model.margin_loss_ids_mixed(ms.formulas, fo, anchors, bad, neg).backward()
    opt.step()
    torch.cuda.synchronize()
    assert int(word.item()) & 1                             # MPQE_FLAG_BAD_NODE_ID
    for k, p in model.named_parameters():
        assert torch.equal(p.detach(), before[k]), k
    model.validate = True
    with pytest.raises(IndexError):
        model.margin_loss_ids_mixed(ms.formulas, fo, anchors, targets, neg)


class Foreign(torch.nn.Module):
    """an encoder that is not the package's: no `table`, no `node_maps`, only the call protocol enc(ids, mode) -> [D, B]"""

    def __init__(self, num_entities, dim):
        super(Foreign, self).__init__()
        self.emb = torch.nn.Embedding(num_entities, dim)

    def forward(self, nodes, mode):
        ids = torch.as_tensor(nodes, dtype=torch.long).to(self.emb.weight.device)
        v = self.emb(ids)
        return (v / v.norm(dim=1, keepdim=True)).t()


@pytest.mark.parametrize('why', ['not fused', 'encode twice', 'learned readout', 'D 20', 'foreign encoder'])
def test_fallbacks_take_the_walk_over_runs(tiny, why, monkeypatch):  # noqa: F811
    index, sets, mixed, model = build(tiny)
    if why == 'learned readout':
        index, sets, mixed, model = build(tiny, 16, 'mlp')
    elif why == 'D 20':
        index, sets, mixed, model = build(tiny, 20, 'mp')           # (scored by the mixed launch, not trained by it)
        assert model._mixed_ok(mixed['2-inter'].formulas, 1)
    model = copy.deepcopy(model)
    if why == 'not fused':
        model.fused = False
    if why == 'encode twice':
        model.encode_twice = True
    if why == 'foreign encoder':
        torch.manual_seed(5)
        model.enc = Foreign(tiny[0].num_entities, model.emb_dim).to('cuda:0')
        assert not model._mixed_ok(mixed['2-inter'].formulas, 1) and model.dropin() is None
    ms, (fo, anchors, targets, neg) = window(mixed, '2-inter')
    mixed_calls, walks = Spy(monkeypatch, ops, 'rgcn_scores_mixed_grad'), Spy(monkeypatch, model_module, 'margin_loss_ids_by_runs')
    got = loss_and_grads(model, lambda: model.margin_loss_ids_mixed(ms.formulas, fo, anchors, targets, neg))
    assert (mixed_calls.n, walks.n) == (0, 1)
    want = loss_and_grads(model, lambda: margin_loss_ids_by_runs(model, ms.formulas, fo, anchors, targets, neg))
    np.testing.assert_allclose(got[0].cpu().numpy(), want[0].cpu().numpy(), **FWD)
    assert all((w is None) == (got[1][k] is None) for k, w in want[1].items())
    if why == 'foreign encoder':        # (the gradients go through the caller's encoder)
        assert got[1]['enc.emb.weight'] is not None and got[1]['enc.emb.weight'].any()


def test_score_ids_is_the_grad_enabled_route_under_no_grad(tiny):  # noqa: F811
    index, sets, mixed, model = build(tiny)
    for qt in ('2-chain', '3-inter'):
        ms = mixed[qt]
        f = int(ms.formula_of_host[0])
        host = ms.offsets_host()
        run = [h for h in range(1, len(ms) + 1) if (ms.formula_of_host[:h] == f).all()][-1]
        neg = (ms.neg[0][:int(host[run])], ms.neg[1][:run + 1])
        a = model.score_ids(ms.formulas[f], ms.anchors[:run], ms.targets[:run], neg=neg)
        with torch.no_grad():
            b = model._score_ids(ms.formulas[f], ms.anchors[:run], ms.targets[:run], neg)
        c = model._score_ids(ms.formulas[f], ms.anchors[:run], ms.targets[:run], neg)
        assert not a.requires_grad and c.requires_grad
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), c.detach().view(torch.int32))


def test_mixed_train_tool_trains_the_rgcn_model_and_is_reproducible():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import train_synthetic
    argv = ['--kg', 'small', '--embed-dim', '32', '--steps', '40', '--device-queries', '--batched-queries', '--mixed-train',
            '--train-queries', '64', '--test-queries', '32']
    runs = [train_synthetic.main(argv) for _ in range(2)]
    curve = np.array(runs[0]['loss_curve'], dtype=np.float64)
    assert runs[0]['mixed_train'] is True and runs[0]['model'] == 'rgcn' and curve.shape == (40,)
    assert curve.tobytes() == np.array(runs[1]['loss_curve'], dtype=np.float64).tobytes()
    assert np.isfinite(curve).all()
    assert curve[-10:].mean() < curve[0]
    with pytest.raises(SystemExit):
        train_synthetic.main(['--mixed-train', '--device-queries', '--readout', 'mlp'])
    with pytest.raises(SystemExit):
        train_synthetic.main(['--mixed-train', '--device-queries', '--dropin'])
