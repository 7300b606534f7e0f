"""State the drop-in (mpqe_amd/dropin.py, csrc/host/autograd_node.cpp, mpqe_amd/optim.py) keeps from one call and one
backward pass to the next, off the happy path of tests/test_dropin_gpu.py -- every iteration checked on its own against a
float64 reference of the same pass (tests/dropin_oracle.py):

  - FlatOptimizer.zero_grad() with passes that are not all drop-in calls: the module path from some iteration on, module-path
    terms beside drop-in calls, a margin_loss too large for the fused step beside fused ones, a pass with no margin_loss;
  - a backward pass that raises after a drop-in node has run, and the passes after it;
  - forward-only calls queued far ahead of the device (their pinned id arenas must outlive the reads);
  - a batch whose anchor_ids are edited in place (collate_fn's copy, the fused path's window check).

Each case runs through the C++ autograd node and through its torch.autograd.Function fallback."""
import random

import numpy as np
import pytest
import torch

from tests.dropin_oracle import FWD, Iteration, adam_state, check_adam, oracle_scores, params64
from tests.test_dropin_gpu import _aifb

pytestmark = pytest.mark.gpu
IMPLS = ('c++', 'python')
MODELS = [(64, 'mp'), (128, 'mp'), (64, 'mlp'), (128, 'mlp')]


def _setup(monkeypatch, impl, D, readout, per_formula=300):
    from mpqe_amd import _lib
    if impl == 'python':
        monkeypatch.setattr(_lib, 'load_autograd_node', lambda: None)
    wd = 1e-3 if readout == 'mlp' else 0.0
    adaptive = readout == 'mp'
    schema, node_maps, model, train_queries = _aifb(readout, adaptive, D=D, per_formula=per_formula, weight_decay=wd)
    model = model.to('cuda:0')
    cfg = dict(readout=readout, scatter_op='add', num_layers=3, adaptive=adaptive, weight_decay=wd)
    d = model.dropin()
    assert d is not None and d.node_impl == impl
    return schema, node_maps, model, train_queries, cfg, d


def _iterators(model, train_queries, B, seed):
    from mpqe_amd.data_utils import get_queries_iterator
    np.random.seed(seed)
    return {qt: get_queries_iterator(train_queries[qt], B, model) for qt in train_queries}


def _loop_body(it, iterators, train_queries, inter_weight=0.005, path_weight=0.01):
    """reference train_helpers.py:81-112 (edge_conv phase), every call recorded by the float64 reference."""
    loss = it.margin_loss(next(iterators['1-chain']))
    for qt in train_queries:
        if qt == '1-chain':
            continue
        if 'inter' in qt:
            loss = loss + it.margin_loss(next(iterators[qt]), weight=inter_weight)
            loss = loss + it.margin_loss(next(iterators[qt]), hard=True, weight=inter_weight)
        else:
            loss = loss + it.margin_loss(next(iterators[qt]), weight=path_weight)
    return loss


def _basis_norm(model):
    return model.layers[0].basis.pow(2).sum()


def _basis_norm64(params):
    return params['layers.0.basis'].pow(2).sum()


def _encode_term(batch):
    """A term through model.encode (the module path's encoder) and its float64 twin."""
    from oracle import ref_cpu
    formula, queries = batch[0], batch[1]

    def dev(model):
        return model.encode(*batch[:5]).pow(2).mean()

    def ref(params, cfg_nm):
        cfg, node_maps, model = cfg_nm
        col = ref_cpu.collate(formula, queries, model.rel_ids, model.mode_ids)
        return ref_cpu.encode_queries(params, cfg, node_maps, formula, col, ref_cpu.rgcn_layer_grouped).pow(2).mean()
    return dev, ref


def _step_and_check(it, opt, model, loss, what):
    value = loss.item()
    loss.backward()
    np.testing.assert_allclose(value, it.reference(), err_msg=what, **FWD)
    it.check_grads(model, what)
    st = adam_state(opt)
    opt.step()
    check_adam(opt, st, what)


@pytest.mark.parametrize('D,readout', MODELS)
@pytest.mark.parametrize('case', ['fused_off', 'module_terms', 'too_large_call', 'no_margin_loss'])
@pytest.mark.parametrize('impl', IMPLS)
def test_flat_adam_zero_grad_with_module_path_terms(impl, case, D, readout, monkeypatch):
    """mpqe_amd.optim.Adam (one flat launch) through iterations whose backward passes are not all drop-in calls. zero_grad()
    must leave every p.grad at zero whatever the pass does: (fused_off) `model.fused = False` from iteration 2 on -- no
    drop-in node at all; (module_terms) a parameter norm and a term through model.encode added to the drop-in calls' loss;
    (too_large_call) one margin_loss beyond the fused step's id limit (the module path) beside fused ones; (no_margin_loss)
    one pass of module-path terms alone. Every iteration's gradients and Adam update against float64."""
    from mpqe_amd import dropin as dropin_mod
    from mpqe_amd import optim
    schema, node_maps, model, train_queries, cfg, d = _setup(monkeypatch, impl, D, readout)
    if case == 'too_large_call':
        monkeypatch.setattr(dropin_mod, 'MAX_IDS', 1000)           # 5 x 300 ids: not covered; 5 x 128: covered
    opt = optim.Adam([p for p in model.parameters() if p.requires_grad], lr=0.01)
    assert opt.flat
    iterators = _iterators(model, train_queries, 128, seed=7)
    big = _iterators(model, train_queries, 300, seed=8)
    random.seed(1234)
    for k in range(4):
        what = '%s iteration %d' % (case, k)
        if case == 'fused_off' and k == 1:
            model.fused = False
        opt.zero_grad()
        it = Iteration(model, cfg, node_maps)
        steps = d.steps
        if case == 'no_margin_loss' and k == 2:
            loss = it.extra(_basis_norm, _basis_norm64, weight=0.5)
        else:
            loss = _loop_body(it, iterators, train_queries)
        if case == 'module_terms' or (case == 'no_margin_loss' and k == 2):
            dev, ref = _encode_term(next(iterators['3-inter_chain']))
            loss = loss + it.extra(_basis_norm, _basis_norm64, weight=0.05)
            loss = loss + it.extra(dev, lambda p: ref(p, (cfg, node_maps, model)), weight=0.3)
        if case == 'too_large_call':
            loss = loss + it.margin_loss(next(big['2-inter']), weight=0.2)
        _step_and_check(it, opt, model, loss, what)
        fused_pass = not (case == 'fused_off' and k >= 1) and not (case == 'no_margin_loss' and k == 2)
        assert (d.steps > steps) == fused_pass, what
    if model.fused:
        d._check_mirror()


class _Boom(torch.autograd.Function):
    """A node whose backward raises (a bad batch in a caller's try/except loop)."""

    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        raise ValueError('boom')


@pytest.mark.parametrize('D,readout', MODELS)
@pytest.mark.parametrize('impl', IMPLS)
def test_passes_after_a_backward_that_raised(impl, D, readout, monkeypatch):
    """A backward pass raises AFTER a drop-in node has run (the engine drops the pass' final callbacks on error): the next
    passes must still flush -- zero_grad and two normal iterations match float64, and the fused step count grows by one
    per pass."""
    from mpqe_amd import optim
    schema, node_maps, model, train_queries, cfg, d = _setup(monkeypatch, impl, D, readout)
    opt = optim.Adam([p for p in model.parameters() if p.requires_grad], lr=0.01)
    iterators = _iterators(model, train_queries, 128, seed=9)
    random.seed(99)
    opt.zero_grad()
    it = Iteration(model, cfg, node_maps)
    _step_and_check(it, opt, model, _loop_body(it, iterators, train_queries), 'first iteration')
    # the failing pass: _Boom's node is made BEFORE the margin_loss call, so it has the lower sequence number and the engine
    # runs it after the drop-in node
    opt.zero_grad()
    x = torch.zeros((), device='cuda:0', requires_grad=True)
    boom = _Boom.apply(x)
    loss = model.margin_loss(*next(iterators['2-inter'])) + boom
    with pytest.raises(ValueError, match='boom'):
        loss.backward()
    # the drop-in node really ran before the raise: its call is waiting for a flush that will never come
    pending = d._pass.pending() if impl == 'c++' else len(d._pending)
    assert pending == 1
    del loss, boom
    steps = d.steps
    for k in range(2):
        opt.zero_grad()
        it = Iteration(model, cfg, node_maps)
        _step_and_check(it, opt, model, _loop_body(it, iterators, train_queries), 'iteration %d after the failed pass' % k)
    assert d.steps == steps + 2
    d._check_mirror()


def _sleep_cycles(ms):
    """torch.cuda._sleep's argument for about `ms` milliseconds on this device (measured)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    probe = 1 << 20
    torch.cuda.synchronize()
    a.record()
    torch.cuda._sleep(probe)
    b.record()
    b.synchronize()
    return int(probe * ms / max(a.elapsed_time(b), 0.05))


@pytest.mark.parametrize('D,readout', [(128, 'mp'), (64, 'mlp')])
@pytest.mark.parametrize('impl', IMPLS)
def test_forward_calls_queued_behind_a_busy_stream(impl, D, readout, monkeypatch):
    """~600 no-grad model.forward calls (the evaluation loops, with `model.validate = False`: no error-word read, so no
    synchronisation per call) issued while the stream is held by a bounded sleep: far more than 17 id arenas are retired
    before the device has read any of them. No arena may be given back while a queued call still reads it -- every call's
    scores against float64, after the fact."""
    from mpqe_amd import ops
    schema, node_maps, model, train_queries, cfg, d = _setup(monkeypatch, impl, D, readout, per_formula=700)
    model.eval()
    model.validate = False
    formula, pool = next(iter(train_queries['3-inter_chain'].items()))
    rng = np.random.RandomState(3)
    B, distinct = 512, 41              # (41 batches: prime to the 16 calls of an arena, so a re-used block holds other ids)
    batches = []
    for _ in range(distinct):
        qs = [pool[i] for i in rng.choice(len(pool), B, replace=False)]
        batches.append((qs, np.array([q.anchor_nodes for q in qs], dtype=np.int64),
                        np.array([q.target_node for q in qs], dtype=np.int64)))
    n_calls = 600
    cycles = _sleep_cycles(80.0)
    outs = []
    with torch.no_grad():
        model.forward(formula, batches[0][0], batches[0][2], anchor_ids=batches[0][1])     # (records made)
        torch.cuda.synchronize()
        arenas, cur = 0, None         # (counted by identity, holding none but the current one)
        torch.cuda._sleep(cycles)
        for k in range(n_calls):
            qs, a, t = batches[k % distinct]
            outs.append(model.forward(formula, qs, t, anchor_ids=a))
            if d._arena is not cur:
                arenas, cur = arenas + 1, d._arena
        cur = None
        torch.cuda.synchronize()
    assert arenas > 17
    ops.raise_on_flags(d.step.err)
    params = params64(model)
    want = [oracle_scores(model, cfg, node_maps, params, formula, qs, t) for qs, _a, t in batches]
    bad = [k for k in range(n_calls) if not np.allclose(outs[k].cpu().numpy(), want[k % distinct], **FWD)]
    assert not bad, 'calls whose scores are not their ids\' (%d of %d): %s' % (len(bad), n_calls, bad[:20])


@pytest.mark.parametrize('D,readout', [(64, 'mp'), (128, 'mlp')])
@pytest.mark.parametrize('impl', IMPLS)
def test_anchor_ids_edited_in_place(impl, D, readout, monkeypatch):
    """A batch's anchor_ids edited in place: later batches of the formula come out as the queries say, and margin_loss on
    the edited batch gives float64's loss and gradients on the EDITED ids -- on the fused path and on the module path."""
    from mpqe_amd.data_utils import get_queries_iterator
    schema, node_maps, model, train_queries, cfg, d = _setup(monkeypatch, impl, D, readout)
    formula, queries = next(iter(train_queries['3-inter'].items()))
    np.random.seed(4)
    it = get_queries_iterator({formula: queries}, 100, model)      # (one formula: windows 0, 100, 200, then 0 again)
    batch = next(it)
    orig = batch[2].clone()
    batch[2][3, 0] = batch[2][5, 0]
    batch[2][17, 2] = batch[2][40, 2]
    for fused in (True, False):
        model.fused = fused
        for p in model.parameters():
            p.grad = None
        random.seed(6)
        ref = Iteration(model, cfg, node_maps)
        loss = ref.margin_loss(batch, weight=0.5)
        value = loss.item()
        loss.backward()
        what = 'fused' if fused else 'module path'
        np.testing.assert_allclose(value, ref.reference(), err_msg=what, **FWD)
        ref.check_grads(model, what)
    model.fused = True
    d._check_mirror()
    later = [next(it) for _ in range(3)]
    np.testing.assert_array_equal(later[-1][2].numpy(), orig.numpy())      # the same window, as the queries hold it
