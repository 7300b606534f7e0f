"""QueryEncoderDecoder (the GQE baseline) on the GPU through its module surface alone: model.forward and
model.margin_loss(...).backward(). Tolerances: tests/gqe_oracle.py FWD / BWD (those of tests/test_configs_gpu.py)."""
import random

import numpy as np
import pytest
import torch

from tests import gqe_common as gc
from tests.gqe_oracle import BWD, FWD

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(params=gc.case_paths(), ids=gc.case_ids())
def case(request):
    return gc.load_case(request.param)


def _loss_and_grads(model, case):
    random.seed(case.meta['loss_seed'])
    model.zero_grad()
    loss = model.margin_loss(case.formula, case.queries, hard_negatives=case.hard_negatives)
    loss.backward()
    grads = {k: (np.zeros(tuple(p.shape), np.float32) if p.grad is None else p.grad.detach().cpu().numpy())
             for k, p in model.named_parameters()}
    return float(loss.item()), grads


def test_fused_reproduces_the_fixtures(case):
    model = gc.build_model(case, DEV)
    a = case.arrays
    targets = a['targets'].tolist()
    plan = model._plan(case.formula)
    assert model.fused is True and model._fused_ok(plan)
    calls = []
    from mpqe_amd import ops
    real = ops.gqe_scores
    ops.gqe_scores = lambda *args, **kw: (calls.append(1), real(*args, **kw))[1]
    try:
        with torch.no_grad():
            s = model.forward(case.formula, case.queries, targets, neg_nodes=a['eval_negs'].tolist(),
                              neg_lengths=a['neg_lengths'].tolist())
            sp = model.forward(case.formula, case.queries, targets)
            sn = model.forward(case.formula, case.queries, a['neg_nodes'].tolist())
        assert len(calls) == 3                        # one fused call per forward
        loss, grads = _loss_and_grads(model, case)
        assert len(calls) == 4                        # ... and one per margin_loss, targets and negatives together
    finally:
        ops.gqe_scores = real
    np.testing.assert_allclose(s.cpu().numpy(), a['eval_scores'], **FWD)
    np.testing.assert_allclose(sp.cpu().numpy(), a['scores_pos'], **FWD)
    np.testing.assert_allclose(sn.cpu().numpy(), a['scores_neg'], **FWD)
    np.testing.assert_allclose(loss, float(a['loss']), **FWD)
    want = case.grads()
    assert set(want) == set(grads)
    for k, g in want.items():
        np.testing.assert_allclose(grads[k], g, err_msg=k, **BWD)


def test_composed_reproduces_the_fixtures(case):
    """fused = False: the decoders' own forward / project, op by op."""
    model = gc.build_model(case, DEV, fused=False)
    a = case.arrays
    with torch.no_grad():
        s = model.forward(case.formula, case.queries, a['targets'].tolist(), neg_nodes=a['eval_negs'].tolist(),
                          neg_lengths=a['neg_lengths'].tolist())
    np.testing.assert_allclose(s.cpu().numpy(), a['eval_scores'], **FWD)
    loss, grads = _loss_and_grads(model, case)
    np.testing.assert_allclose(loss, float(a['loss']), **FWD)
    for k, g in case.grads().items():
        np.testing.assert_allclose(grads[k], g, err_msg=k, **BWD)


def test_decoders_work_on_their_own(case):
    """BilinearMetapathDecoder.forward / project and the intersection decoders called directly, columns in, columns out, against
    the same products in torch."""
    model = gc.build_model(case, DEV, fused=False)
    D = case.D
    g = torch.Generator().manual_seed(3)
    e1, e2, e3 = (torch.randn(D, 7, generator=g).to(DEV) for _ in range(3))
    rel = next(iter(model.path_dec.mats))
    M = model.path_dec.mats[rel].detach()
    np.testing.assert_allclose(model.path_dec.project(e1, rel).detach().cpu().numpy(), (M @ e1).cpu().numpy(), rtol=1e-4, atol=1e-5)
    if rel[0] == rel[2]:
        rels = (rel, rel)
    else:
        rels = (rel,)
    act = e1.t()
    for r in rels:
        act = act @ model.path_dec.mats[r].detach()
    want = torch.nn.functional.cosine_similarity(act.t(), e2, dim=0)
    np.testing.assert_allclose(model.path_dec.forward(e1, e2, rels).detach().cpu().numpy(), want.cpu().numpy(), rtol=1e-4, atol=1e-5)
    mode = case.modes[0]
    for third in ([], e3):
        got = model.inter_dec(e1, e2, mode, third)
        xs = [e1, e2] + ([third] if len(third) else [])
        if not case.cfg['inter'].endswith('simple'):
            xs = [torch.relu(model.inter_dec.pre_mats[mode].detach() @ x) for x in xs]
        st = torch.stack(xs)
        c = st.mean(0) if case.cfg['inter'].startswith('mean') else st.min(0)[0]
        if not case.cfg['inter'].endswith('simple'):
            c = model.inter_dec.post_mats[mode].detach() @ c
        np.testing.assert_allclose(got.detach().cpu().numpy(), c.cpu().numpy(), rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize('qt,inter', [('3-chain', 'mean'), ('3-inter_chain', 'min')])
def test_fused_against_composed_and_oracle(qt, inter):
    """D = 128, B = 33 (a tile tail, three workgroups), ragged negatives: fused = True against fused = False and both against
    the float64 oracle."""
    from mpqe_amd.data_utils import make_feature_modules
    from mpqe_amd.encoders import DirectEncoder
    from mpqe_amd.model import QueryEncoderDecoder
    from mpqe_amd.utils import get_intersection_decoder, get_metapath_decoder
    prob, o, scores = gc.settled_problem(qt, 128, 33, inter, 11)

    class G(object):
        relations = {a: [(b, name) for name in gc.NAMES for b in gc.MODES] for a in gc.MODES}
        full_lists = {m: prob.ids[m].tolist() for m in gc.MODES}
    fm, node_maps = make_feature_modules(prob.ids, 128, prob.node_map.shape[0] - 1)
    assert np.array_equal(node_maps.numpy(), prob.node_map)
    dims = {m: 128 for m in gc.MODES}
    model = QueryEncoderDecoder(G(), DirectEncoder(None, fm, node_maps), get_metapath_decoder(G(), dims, 'bilinear'),
                                get_intersection_decoder(G(), dims, inter))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in prob.params.items()}, strict=True)
    model = model.to(DEV)
    queries = [type('Q', (), {'anchor_nodes': tuple(int(v) for v in row)})() for row in prob.anchors]
    gs = torch.from_numpy(prob.grad_scores).to(DEV)
    out = {}
    for fused in (True, False):
        model.fused = fused
        model.zero_grad()
        s = model.forward(prob.formula, queries, prob.targets.tolist(), neg_nodes=prob.negs.tolist(),
                          neg_lengths=prob.neg_lengths.tolist())
        s.backward(gs)
        out[fused] = (s.detach().cpu().numpy(), {k: p.grad.detach().cpu().numpy().copy() for k, p in model.named_parameters()
                                                 if p.grad is not None})
    for fused in (True, False):
        s, grads = out[fused]
        np.testing.assert_allclose(s, scores, err_msg='fused=%s' % fused, **FWD)
        for k, g in grads.items():
            np.testing.assert_allclose(g, o.grads[k], err_msg='fused=%s %s' % (fused, k), **BWD)
    np.testing.assert_allclose(out[True][0], out[False][0], **FWD)
    assert set(out[True][1]) == set(out[False][1])
    for k in out[True][1]:
        np.testing.assert_allclose(out[True][1][k], out[False][1][k], err_msg=k, **BWD)


def test_evaluation_loops_equal_the_oracle(case):
    from mpqe_amd import evaluation
    model = gc.build_model(case, DEV)
    o = gc.case_oracle(case)

    class OracleModel(object):
        def forward(self, formula, queries, targets, neg_nodes=None, neg_lengths=None):
            anchors = [q.anchor_nodes for q in queries]
            return torch.from_numpy(o.forward(formula, anchors, targets, neg_nodes, neg_lengths, case.cfg['inter']))
    tq = {case.formula: case.queries}
    with torch.no_grad():
        auc, per = evaluation.eval_auc_queries(tq, model, batch_size=2, seed=3)
        perc = evaluation.eval_perc_queries(tq, model, batch_size=2)
    auc_o, per_o = evaluation.eval_auc_queries(tq, OracleModel(), batch_size=2, seed=3)
    perc_o = evaluation.eval_perc_queries(tq, OracleModel(), batch_size=2)
    assert auc == auc_o and per == per_o
    assert perc == perc_o


def test_bad_id_raises_index_error(case):
    model = gc.build_model(case, DEV)
    targets = case.arrays['targets'].tolist()
    targets[0] = case.num_entities                 # in node_maps, of no mode
    with pytest.raises(IndexError):
        with torch.no_grad():
            model.forward(case.formula, case.queries, targets)
    with torch.no_grad():                          # the word is cleared: the next call is clean
        model.forward(case.formula, case.queries, case.arrays['targets'].tolist())


def _train(opt_cls, steps=20):
    from mpqe_amd import synthetic
    from mpqe_amd.data_utils import make_feature_modules
    from mpqe_amd.encoders import DirectEncoder
    from mpqe_amd.model import QueryEncoderDecoder
    from mpqe_amd.utils import get_intersection_decoder, get_metapath_decoder
    D, B = 32, 48
    schema = synthetic.make_schema(*synthetic.KG_SHAPES['tiny'], seed=5)
    torch.manual_seed(5)
    graph = synthetic.SchemaGraph(schema, D)
    graph.full_lists = {m: [int(v) for v in ids] for m, ids in graph.full_lists.items()}
    fm, node_maps = make_feature_modules(schema.ids, D, schema.num_entities)
    dims = {m: D for m in schema.modes}
    model = QueryEncoderDecoder(graph, DirectEncoder(None, fm, node_maps), get_metapath_decoder(graph, dims, 'bilinear'),
                                get_intersection_decoder(graph, dims, 'min')).to(DEV)
    rng = np.random.RandomState(6)
    batches = []
    for qt in ('1-chain', '2-chain', '2-inter', '3-inter_chain', '3-chain_inter'):
        f = synthetic.sample_formula(schema, qt, rng)
        batches.append((f, synthetic.sample_queries(schema, f, B, rng, n_neg=4, n_hard=2)))
    opt = opt_cls(model.parameters(), lr=0.01)
    random.seed(7)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss = model.margin_loss(*batches[0])
        for f, qs in batches[1:]:
            loss = loss + model.margin_loss(f, qs, hard_negatives='inter' in f.query_type)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    return losses, {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}


@pytest.mark.parametrize('which', ['torch', 'mpqe_amd'])
def test_training_lowers_the_loss_and_repeats_bit_for_bit(which):
    from mpqe_amd import optim
    opt_cls = torch.optim.Adam if which == 'torch' else optim.Adam
    losses, params = _train(opt_cls)
    means = [float(np.mean(losses[i:i + 5])) for i in range(0, 20, 5)]
    print('5-step means of the loss:', means)
    assert all(b < a for a, b in zip(means, means[1:])), means
    losses2, params2 = _train(opt_cls)
    assert losses == losses2
    for k in params:
        assert params[k].tobytes() == params2[k].tobytes(), k
