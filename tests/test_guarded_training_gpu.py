"""A step whose error word is set is not applied (FlatOptimizer(guard=True), mpqe_amd.optim.Adam / SGD): the unchecked
training loops hear of a bad entity id one call late, AFTER optimizer.step() -- the update's launches read the word on the
device and write nothing, so the parameters and both Adam moments are those of the last good step, and training goes on
from there bit for bit as if the bad step had never been queued.

Shapes. The comparisons against a control run are bit for bit, so they run where the step's sums have one order: the chain
form, whose smallest embedding dimension is 64 (below it the level form adds the entity-table gradients with fp32 atomics,
whose order differs from run to run; row-sparse tables exist on the chain form only). The refusal itself -- untouched
buffers, the device's count, IndexError -- does not depend on the form and is checked at D = 32 too. 16 graphs a batch."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _setup(D, B=16, seed=0):
    from mpqe_amd import synthetic
    from mpqe_amd.data_utils import make_feature_modules
    from mpqe_amd.encoders import DirectEncoder
    from mpqe_amd.model import RGCNEncoderDecoder
    torch.manual_seed(seed)
    schema = synthetic.make_schema(*synthetic.KG_SHAPES['tiny'], seed=seed)
    graph = synthetic.SchemaGraph(schema, D)
    fm, node_maps = make_feature_modules(schema.ids, D, schema.num_entities)
    model = RGCNEncoderDecoder(graph, DirectEncoder(None, fm, node_maps), readout='mp', num_layers=3,
                               shared_layers=False, adaptive=True, weight_decay=0).to('cuda:0')
    with torch.no_grad():
        for p in model.layers.parameters():
            p.mul_(5.0)
    rng = np.random.RandomState(seed + 1)
    batches = []
    for qt, hard in synthetic.FULL_MIX:
        f = synthetic.sample_formula(schema, qt, rng)
        qs = synthetic.sample_queries(schema, f, B, rng)
        batches.append(dict(formula=f, queries=qs, weight=float(rng.uniform(0.1, 1.0)),
                            anchor_ids=np.array([q.anchor_nodes for q in qs], dtype=np.int64),
                            targets=np.array([q.target_node for q in qs], dtype=np.int64),
                            negs=np.array([q.neg_samples[0] for q in qs], dtype=np.int64)))
    return model, batches


def _with_bad_id(batches):
    bad = [dict(b) for b in batches]
    bad[3]['negs'] = bad[3]['negs'].copy()
    bad[3]['negs'][5] = 10 ** 6                              # outside the id -> row table
    return bad


def _state(opt):
    torch.cuda.synchronize()
    return [t.clone() for t in (opt.flat_param, opt.exp_avg, opt.exp_avg_sq) if t is not None]


def _same_bits(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), '%s: buffer %d differs' % (what, i)


def _make(kind, D, guard=True):
    from mpqe_amd.fused import FusedTrainStep
    from mpqe_amd.optim import FlatOptimizer
    model, batches = _setup(D)
    sparse = kind == 'adam_sparse'
    step = FusedTrainStep(model, sparse_tables=sparse)
    opt = FlatOptimizer(step, lr=0.01, opt='sgd' if kind == 'sgd' else 'adam', sparse_tables=sparse, guard=guard)
    return step, opt, batches


def _one(step, opt, batches):
    packed = step.pack(batches)
    step.run(packed)                              # unchecked: the host does not look at the error word
    opt.step(packed) if opt.sparse_tables else opt.step()
    torch.cuda.synchronize()


@pytest.mark.parametrize('kind', ['adam', 'sgd', 'adam_sparse'])
def test_flagged_step_is_not_applied_and_training_continues(kind):
    step, opt, batches = _make(kind, 64)
    assert step.uses_chain(step.pack(batches))
    _one(step, opt, batches)
    _one(step, opt, batches)
    snap = _state(opt)
    _one(step, opt, _with_bad_id(batches))        # the step flags the id; the update runs before anyone has asked
    _same_bits(_state(opt), snap, 'after the refused update')
    assert opt.steps_applied() == 2
    with pytest.raises(IndexError):
        step.check()
    _one(step, opt, batches)
    _one(step, opt, batches)
    assert opt.steps_applied() == 4 and opt.t == 4
    step.check()
    final = _state(opt)
    assert not torch.equal(final[0], snap[0])
    # the control: the four good steps alone, from the same seed
    cstep, copt, cbatches = _make(kind, 64)
    for _ in range(4):
        _one(cstep, copt, cbatches)
    cstep.check()
    assert copt.steps_applied() == 4
    _same_bits(final, _state(copt), 'against the control run')


@pytest.mark.parametrize('kind', ['adam', 'sgd'])
def test_flagged_step_is_not_applied_small_dimension(kind):
    """D = 32 (the level form): the refusal, the count, the late IndexError, and the update after the host has cleared the
    word uses t = applied + 1."""
    step, opt, batches = _make(kind, 32)
    _one(step, opt, batches)
    _one(step, opt, batches)
    snap = _state(opt)
    _one(step, opt, _with_bad_id(batches))
    _one(step, opt, batches)                      # the word is sticky: a good step behind an unread fault is refused too
    _same_bits(_state(opt), snap, 'after the refused updates')
    assert opt.steps_applied() == 2 and opt.t == 4          # (the host has counted on: it has not been told yet)
    with pytest.raises(IndexError):
        step.check()
    _one(step, opt, batches)
    assert opt.steps_applied() == 3 and opt.t == 3
    assert not torch.equal(_state(opt)[0], snap[0])
    step.check()


def test_guard_off_gives_the_same_bits_on_clean_steps():
    out = {}
    for guard in (True, False):
        step, opt, batches = _make('adam', 64, guard=guard)
        for _ in range(3):
            _one(step, opt, batches)
        step.check()
        out[guard] = _state(opt)
        assert opt.t == 3
        if guard:
            assert opt.steps_applied() == 3
        else:
            assert opt.applied is None
            with pytest.raises(ValueError):
                opt.steps_applied()
    _same_bits(out[True], out[False], 'guard=True against guard=False')


def test_drop_in_loop_refuses_the_flagged_iteration():
    """The reference's loop body (train_helpers.py:78-120: zero_grad, margin_loss per query type, loss.backward(),
    optimizer.step()) with `from mpqe_amd import optim`. One iteration's last margin_loss holds a query with a bad anchor
    id: its optimizer.step() changes nothing, the next margin_loss raises IndexError, and training goes on to the bits of
    the control without that iteration."""
    from mpqe_amd import optim
    from mpqe_amd.data_utils import get_queries_iterator
    from tests.test_dropin_gpu import _aifb

    def run(with_bad):
        schema, node_maps, model, train_queries = _aifb('mp', True, D=64, per_formula=80, kg='tiny')
        model = model.to('cuda:0')
        opt = optim.Adam([p for p in model.parameters() if p.requires_grad], lr=0.01)
        assert opt.flat and opt._impl.guard
        np.random.seed(4)
        its = {qt: get_queries_iterator(train_queries[qt], 16, model) for qt in ('1-chain', '2-inter')}
        drawn = [(next(its['1-chain']), next(its['2-inter'])) for _ in range(4)]

        def iteration(a, b, seed):
            random.seed(seed)
            opt.zero_grad()
            loss = model.margin_loss(*a)
            loss += 0.005 * model.margin_loss(*b)
            loss.backward()
            opt.step()
            torch.cuda.synchronize()

        for i, (a, b) in enumerate(drawn):
            if with_bad and i == 2:
                before = _state(opt._impl)
                bad_anchors = b[2].clone()
                bad_anchors[7, 1] = schema.num_entities + 11
                iteration(a, (b[0], list(b[1]), bad_anchors), 999)
                _same_bits(_state(opt._impl), before, 'after the flagged iteration')
                with pytest.raises(IndexError):
                    random.seed(100 + i)
                    model.margin_loss(*a)
            iteration(a, b, 100 + i)
        model.dropin()._check_mirror()
        assert opt._impl.steps_applied() == 4 and opt._impl.t == 4
        return _state(opt._impl)

    _same_bits(run(True), run(False), 'against the control loop')
