"""A float64 reference of ONE training iteration through the drop-in entry points (mpqe_amd/dropin.py), for tests that
keep state from one call and one backward pass to the next.

    it = Iteration(model, cfg, node_maps)            # the device parameters, now, as float64 CPU tensors
    loss = it.margin_loss(batch, weight=1.0)         # model.margin_loss(*batch) recorded; returns weight * its value
    loss = loss + it.extra(dev_fn, ref_fn)           # any other term of the pass: dev_fn(model), ref_fn(params64)
    loss.backward()
    it.check_grads(model)                            # every p.grad against the float64 gradient of the same pass
    before = adam_state(opt)                         # the flat optimiser's state just before its step
    opt.step()
    check_adam(opt, before)                          # the update against a float64 Adam from that state

The negatives are replayed from python's `random` stream with the reference's own expressions (model.py:470-476), so each
iteration is checked on its own: a stale gradient sum, a wiped term or a missing flush is a factor of 2 or a missing
contribution, never drift.
"""
import random

import numpy as np
import torch

from oracle import ref_cpu

BWD = dict(rtol=1e-4, atol=2e-6)        # tests/test_dropin_gpu.py's gradient tolerances
FWD = dict(rtol=1e-5, atol=1e-6)


def params64(model):
    """The model's parameters as float64 CPU leaves, keyed like ref_cpu's params."""
    return {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in model.state_dict().items()}


def collate64(model, formula, queries, anchor_ids=None):
    col = ref_cpu.collate(formula, queries, model.rel_ids, model.mode_ids)
    if anchor_ids is not None:
        col['anchor_ids'] = np.array(anchor_ids, dtype=np.int64).reshape(col['B'], col['A'])
    return col


def draw_negatives(model, formula, queries, hard):
    """reference model.py:466-476 on python's global stream."""
    if hard:
        return [random.choice(q.hard_neg_samples) for q in queries]
    if formula.query_type == '1-chain':
        return [random.choice(model.graph.full_lists[formula.target_mode]) for _ in queries]
    return [random.choice(q.neg_samples) for q in queries]


class Iteration(object):
    def __init__(self, model, cfg, node_maps):
        self.model, self.cfg, self.node_maps = model, cfg, node_maps
        self.params = params64(model)
        self.state = random.getstate()
        self.terms = []
        self.value = None

    def margin_loss(self, batch, hard=False, margin=1, weight=1.0):
        formula, queries, anchor_ids = batch[0], batch[1], batch[2] if len(batch) > 2 else None
        # (the ids as the batch holds them at the call: a caller may have edited them)
        a = None if anchor_ids is None else anchor_ids.detach().cpu().numpy().copy()
        self.terms.append(('margin', weight, (formula, list(queries), a, hard, float(margin))))
        out = self.model.margin_loss(*batch, hard_negatives=hard, margin=margin)
        return out if weight == 1.0 else weight * out

    def extra(self, dev_fn, ref_fn, weight=1.0):
        self.terms.append(('extra', weight, ref_fn))
        out = dev_fn(self.model)
        return out if weight == 1.0 else weight * out

    def reference(self):
        """The float64 loss of the recorded pass (its gradient lands on self.params' .grad). python's stream is left
        where the device pass left it -- and must have been left there by exactly the reference's draws."""
        after = random.getstate()
        random.setstate(self.state)
        total = torch.zeros((), dtype=torch.float64)
        for kind, w, t in self.terms:
            if kind == 'margin':
                formula, queries, a, hard, margin = t
                negs = draw_negatives(self.model, formula, queries, hard)
                col = collate64(self.model, formula, queries, a)
                targets = np.array([q.target_node for q in queries])
                l = ref_cpu.margin_loss(self.params, self.cfg, self.node_maps, formula, col, targets, np.array(negs),
                                        margin=margin, layer_fn=ref_cpu.rgcn_layer_grouped, encode_twice=False)
            else:
                l = t(self.params)
            total = total + w * l
        assert random.getstate() == after, 'the device pass drew other negatives than the reference'
        for p in self.params.values():
            p.grad = None
        total.backward()
        self.value = total.item()
        return self.value

    def check_grads(self, model, what=''):
        """Every p.grad of `model` against the float64 gradient of the recorded pass (None = zero on both sides)."""
        if self.value is None:
            self.reference()
        for k, p in model.named_parameters():
            r = self.params[k].grad
            r = np.zeros(tuple(p.shape)) if r is None else r.numpy()
            g = np.zeros(tuple(p.shape), np.float32) if p.grad is None else p.grad.detach().cpu().numpy()
            np.testing.assert_allclose(g, r, err_msg='%s %s' % (what, k), **BWD)


def oracle_scores(model, cfg, node_maps, params, formula, queries, targets):
    """reference model.py:400-462 (positives only) in float64."""
    col = collate64(model, formula, queries)
    with torch.no_grad():
        return ref_cpu.forward(params, cfg, node_maps, formula, col, np.asarray(targets),
                               layer_fn=ref_cpu.rgcn_layer_grouped).numpy()


# ------------------------------------------------------------------------------------------- the optimiser step
def flat_impl(opt):
    """mpqe_amd.optim.Adam / SGD over one fused model: its FlatOptimizer."""
    impl = getattr(opt, '_impl', opt)
    assert hasattr(impl, 'flat_param'), 'not the flat optimiser'
    return impl


def adam_state(opt):
    """What the flat optimiser's step starts from, as float64 CPU arrays: parameters, gradient, moments, step count."""
    o = flat_impl(opt)
    torch.cuda.synchronize()
    st = dict(p=o.flat_param.detach().cpu().double(), g=o.fused.flat_grad.detach().cpu().double(), t=o.t)
    if o.opt == 'adam':
        st['m'], st['v'] = o.exp_avg.cpu().double(), o.exp_avg_sq.cpu().double()
    return st


def check_adam(opt, st, what=''):
    """The step just taken against torch.optim.Adam's / SGD's rule in float64 from the state `st` held before it."""
    o = flat_impl(opt)
    assert o.t == st['t'] + 1
    p, g = st['p'], st['g']
    if o.weight_decay:
        g = g + o.weight_decay * p
    if o.opt == 'adam':
        b1, b2 = o.betas
        t = o.t
        m = b1 * st['m'] + (1 - b1) * g
        v = b2 * st['v'] + (1 - b2) * g * g
        denom = v.sqrt() / np.sqrt(1 - b2 ** t) + o.eps
        want = p - (o.lr / (1 - b1 ** t)) * m / denom
        np.testing.assert_allclose(o.exp_avg.cpu().numpy(), m.numpy(), rtol=1e-5, atol=1e-9, err_msg=what + ' exp_avg')
        np.testing.assert_allclose(o.exp_avg_sq.cpu().numpy(), v.numpy(), rtol=1e-5, atol=1e-12,
                                   err_msg=what + ' exp_avg_sq')
    else:
        want = p - o.lr * g
    np.testing.assert_allclose(o.flat_param.detach().cpu().numpy(), want.numpy(), rtol=1e-5, atol=1e-7,
                               err_msg=what + ' parameters')
