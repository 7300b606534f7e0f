"""Answering a query with the GQE baseline (QueryEncoderDecoder.answer / rank_targets, evaluation.eval_rank_queries)
against its existing scoring path, model.forward: same scores, same ranks, ids of the target mode only -- on the fused
path (ops.gqe_embed + ops.rank_entities) and on the composed one (fused = False). Modelled on tests/test_answer_gpu.py:
its tolerance (2e-6 + 1e-5 |s|), `close`, `bracket` and `forward_all`.

Every fixture tests/golden/gqe_*.npz (D = 16, B = 5, 20 entities per mode) and a D = 64 model on the small synthetic KG
wired as tools/train_synthetic.py: run_gqe wires it (seed 0, untrained), one chain and one intersection formula, 50
queries each."""
import argparse
import copy
import os
import sys

import numpy as np
import pytest
import torch

from tests import gqe_common as gc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'


def tol(s):
    return 2e-6 + 1e-5 * np.abs(s)


def close(a, b, what=''):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert (np.abs(a - b) <= tol(b)).all(), '%s: worst |diff| %.3g' % (what, np.abs(a - b).max())


def mode_ids(model, mode):
    return np.asarray(list(model.graph.full_lists[mode]), dtype=np.int64)


def forward_all(model, formula, queries, ids):
    """[B, len(ids)] scores of every listed entity through the existing path (ragged negatives of model.forward)."""
    B = len(queries)
    with torch.no_grad():
        s = model.forward(formula, queries, [q.target_node for q in queries], neg_nodes=np.tile(ids, B).tolist(),
                          neg_lengths=[len(ids)] * B)
    return s[B:].reshape(B, len(ids)).cpu().numpy()


def bracket(scores, ids, target, banned=()):
    """lo / hi of the rank of `target` from one query's fp32 scores of all entities, widened by 2 tol."""
    st = float(scores[ids == target][0])
    keep = np.array([i != target and i not in banned for i in ids])
    so = scores[keep].astype(np.float64)
    return 1 + int((so > st + 2 * tol(st)).sum()), 1 + int((so >= st - 2 * tol(st)).sum())


_SCORES = {}


def golden(name, fused):
    """(case, model, ids of the target mode, forward()'s scores of every entity: computed once per fixture and path)."""
    if (name, fused) not in _SCORES:
        case = gc.load_case([p for p in gc.case_paths() if os.path.basename(p)[:-4] == name][0])
        model = gc.build_model(case, DEV, fused=fused).eval()
        ids_all = mode_ids(model, case.formula.target_mode)
        _SCORES[(name, fused)] = (case, model, ids_all, forward_all(model, case.formula, case.queries, ids_all))
    return _SCORES[(name, fused)]


def check_answer(model, f, qs, ids_all, k):
    ids, scores = model.answer(f, qs, k=k)
    assert ids.shape == (len(qs), k) and ids.dtype == torch.int64 and scores.dtype == torch.float32
    assert not ids.requires_grad and not scores.requires_grad
    ids_h, sc_h = ids.cpu().numpy(), scores.cpu().numpy()
    assert np.isin(ids_h, ids_all).all(), 'ids of the target mode only'
    for j in range(k):
        with torch.no_grad():
            ref = model.forward(f, qs, ids_h[:, j].tolist()).cpu().numpy()
        close(sc_h[:, j], ref, 'column %d' % j)


def check_beyond_the_mode(model, f, qs, ids_all):
    # k beyond the mode: -1 / -inf exactly past the eligible count; exclusions honoured
    big = len(ids_all) + 5
    excl = [list(ids_all[i % 3: i % 3 + 4]) for i in range(len(qs))]
    ids2, sc2 = model.answer(f, qs, k=big, exclude=excl)
    ids2, sc2 = ids2.cpu().numpy(), sc2.cpu().numpy()
    n = len(ids_all) - 4
    assert (ids2[:, :n] >= 0).all() and (ids2[:, n:] == -1).all() and np.isneginf(sc2[:, n:]).all()
    assert np.isfinite(sc2[:, :n]).all()
    for i in range(len(qs)):
        assert sorted(ids2[i, :n].tolist()) == sorted(set(ids_all.tolist()) - set(excl[i]))


def check_ranks(model, f, qs, ids_all, s, excl, k):
    ranks = model.rank_targets(f, qs).cpu().numpy()
    ranks_x = model.rank_targets(f, qs, exclude=excl).cpu().numpy()
    for i, q in enumerate(qs):
        lo, hi = bracket(s[i], ids_all, q.target_node)
        assert lo <= ranks[i] <= hi, (i, ranks[i], lo, hi)
        lo, hi = bracket(s[i], ids_all, q.target_node, set(excl[i]))
        assert lo <= ranks_x[i] <= hi, (i, ranks_x[i], lo, hi)
    # exact: the target sits at its rank in answer()
    top, sc = model.answer(f, qs, k=k)
    top, sc = top.cpu().numpy(), sc.cpu().numpy()
    order = np.argsort(ids_all)
    for i, q in enumerate(qs):
        if ranks[i] <= k:
            assert top[i, ranks[i] - 1] == q.target_node
        pos = order[np.searchsorted(ids_all[order], top[i])]
        close(sc[i], s[i][pos], 'scores of query %d' % i)
    return ranks, ranks_x


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'composed'])
@pytest.mark.parametrize('name', gc.case_ids())
def test_answer_scores_and_ids_match_forward(name, fused):
    case, model, ids_all, s = golden(name, fused)
    plan = model._plan(case.formula)
    assert bool(model._fused_ok(plan)) == fused
    check_answer(model, case.formula, case.queries, ids_all, 7)
    check_beyond_the_mode(model, case.formula, case.queries, ids_all)


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'composed'])
@pytest.mark.parametrize('name', gc.case_ids())
def test_rank_targets_matches_ranks_from_forward(name, fused):
    case, model, ids_all, s = golden(name, fused)
    qs = case.queries
    excl = [list(ids_all[i % 5: i % 5 + 6]) + [q.target_node] for i, q in enumerate(qs)]
    ranks, _ = check_ranks(model, case.formula, qs, ids_all, s, excl, len(ids_all))
    assert (ranks <= len(ids_all)).all()


def test_all_fifteen_fixtures_are_covered():
    assert len(gc.case_ids()) == 15


# ---------------------------------------------------------------------------------------------- D = 64 on the small KG
@pytest.fixture(scope='module')
def synth():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import train_synthetic
    args = argparse.Namespace(kg='small', embed_dim=64, batch_size=64, steps=300, lr=0.01, readout='mp', degree=2,
                              formulas=2, train_queries=256, test_queries=96, weight_scale=1.0, seed=0, oracle=False,
                              eval_every=0, decoder='bilinear', inter_decoder='mean')
    schema, graph, node_maps, model, train, test = train_synthetic.build_gqe(args, torch.device(DEV))
    tq_all = train_synthetic.test_dict(test)
    chain = [f for f in tq_all if f.query_type == '2-chain'][0]
    inter = [f for f in tq_all if f.query_type == '3-inter_chain'][0]
    tq = {f: tq_all[f][:50] for f in (chain, inter)}
    known = train_synthetic.known_answers(args, schema, tq)
    return argparse.Namespace(args=args, schema=schema, graph=graph, model=model.eval(), tq=tq, known=known, chain=chain,
                              inter=inter, mod=train_synthetic)


def fresh_twin(synth):
    """A second model of the same wiring with the first one's state loaded."""
    twin = synth.mod.build_gqe(synth.args, torch.device(DEV))[3]
    twin.load_state_dict(synth.model.state_dict())
    return twin.eval()


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'composed'])
def test_synthetic_scores_ranks_and_filtered_evaluation(synth, fused):
    from mpqe_amd import evaluation
    model, tq, known = synth.model, synth.tq, synth.known
    model.fused = fused
    try:
        raw = evaluation.eval_rank_queries(tq, model, batch_size=128, ks=(1, 3, 10))
        filt = evaluation.eval_rank_queries(tq, model, batch_size=128, ks=(1, 3, 10), known_answers=known)
        all_raw, all_filt = [], []
        for f in tq:
            qs = tq[f]
            assert len(qs) == 50 and bool(model._fused_ok(model._plan(f))) == fused
            ids_all = mode_ids(model, f.target_mode)
            s = forward_all(model, f, qs, ids_all)
            k = min(128, len(ids_all))
            assert k == len(ids_all), 'the small KG: every entity of the mode is returned, so every query reaches the exact checks'
            check_answer(model, f, qs, ids_all, 7)
            check_beyond_the_mode(model, f, qs[:9], ids_all)
            r_raw, r_filt = check_ranks(model, f, qs, ids_all, s, [list(known[q]) for q in qs], k)
            assert (r_filt <= r_raw).all()
            top = model.answer(f, qs, k=k)[0].cpu().numpy()
            for i, q in enumerate(qs):
                ahead = set(top[i, :r_raw[i] - 1].tolist())
                assert r_filt[i] == r_raw[i] - len(ahead & (set(known[q]) - {q.target_node}))
            all_raw.extend(r_raw.tolist())
            all_filt.extend(r_filt.tolist())
            np.testing.assert_allclose(filt['per_formula'][f]['mrr'], np.mean(1.0 / r_filt), rtol=1e-12)
            np.testing.assert_allclose(raw['per_formula'][f]['mrr'], np.mean(1.0 / r_raw), rtol=1e-12)
        for out, r in ((raw, np.array(all_raw, dtype=np.float64)), (filt, np.array(all_filt, dtype=np.float64))):
            np.testing.assert_allclose(out['mrr'], np.mean(1.0 / r), rtol=1e-12)
            for k in (1, 3, 10):
                np.testing.assert_allclose(out['hits@%d' % k], np.mean(r <= k), rtol=1e-12)
        assert filt['mrr'] >= raw['mrr']
    finally:
        model.fused = True


def test_chain_candidates_are_projected_once_and_follow_the_parameters(synth, monkeypatch):
    from mpqe_amd import ops
    model, f = synth.model, synth.chain
    qs = synth.tq[f]
    calls = []
    real = ops.gqe_embed

    def counted(*args, **kwargs):
        calls.append(1)
        return real(*args, **kwargs)
    monkeypatch.setattr(ops, 'gqe_embed', counted)
    model.__dict__['_cand'] = None
    model.eval()
    a = model.rank_targets(f, qs)
    b = model.rank_targets(f, qs[:20])
    assert len(calls) == 1, 'eval(): the mode is projected once'
    assert torch.equal(a[:20], b) and torch.equal(a, model.rank_targets(f, qs))
    assert len(calls) == 1
    twin_copy = copy.deepcopy(model)
    assert twin_copy.__dict__.get('_cand') is None and twin_copy.__dict__.get('_row_ids') is None, \
        'the cached projection and row maps are not copied'
    rel = tuple(f.rels[0])
    try:
        with torch.no_grad():
            model.path_dec.mats[rel].mul_(-1)
        c = model.rank_targets(f, qs)
        assert len(calls) == 2, 'a parameter written in place: the next call projects again'
        n_before = len(calls)
        assert torch.equal(c, fresh_twin(synth).rank_targets(f, qs))
        assert len(calls) == n_before + 1           # (the fresh model's own projection)
        assert not torch.equal(a, c), 'the first matrix of the chain, negated: the scores change sign'
    finally:
        with torch.no_grad():
            model.path_dec.mats[rel].mul_(-1)
    assert torch.equal(model.rank_targets(f, qs), a)
    model.train()
    try:
        n0 = len(calls)
        t1 = model.rank_targets(f, qs)
        t2 = model.rank_targets(f, qs)
        assert len(calls) == n0 + 2 and model.__dict__.get('_cand') is None, 'train(): nothing is cached'
        assert torch.equal(t1, a) and torch.equal(t2, a)
    finally:
        model.eval()


def test_copies_device_moves_errors_and_repeats(synth):
    model = synth.model
    for f in (synth.chain, synth.inter):
        qs = synth.tq[f][:33]
        ids, sc = model.answer(f, qs, k=9)
        ids_again, sc_again = model.answer(f, qs, k=9)
        assert torch.equal(ids, ids_again) and torch.equal(sc, sc_again), 'two answer calls give the same bits'
        ranks = model.rank_targets(f, qs)
        twin = copy.deepcopy(model)
        for m in (twin, model.to('cpu').to(DEV)):
            ids2, sc2 = m.answer(f, qs, k=9)
            assert torch.equal(ids, ids2) and torch.equal(sc, sc2) and torch.equal(ranks, m.rank_targets(f, qs))
        other = [m for m in synth.schema.modes if m != f.target_mode][0]
        with pytest.raises(IndexError):
            model.rank_targets(f, qs, target_nodes=[int(synth.schema.ids[other][0])] * len(qs))
        with pytest.raises(IndexError):
            model.answer(f, qs, k=3, exclude=[[int(synth.schema.ids[other][1])]] * len(qs))
        with pytest.raises(ValueError):
            model.answer(f, qs, k=0)
        with pytest.raises(ValueError):
            model.answer(f, qs, k=3, exclude=[[]] * (len(qs) - 1))
        with pytest.raises(ValueError):
            model.rank_targets(f, qs, exclude=[[]] * (len(qs) + 1))
        # (the error word is clean again: the next call answers)
        assert torch.equal(model.rank_targets(f, qs), ranks)

        class Foreign(torch.nn.Module):
            def forward(self, nodes, mode):
                return torch.zeros(64, len(nodes), device=DEV)
        twin.enc = Foreign()
        with pytest.raises(NotImplementedError):
            twin.answer(f, qs, k=3)
        with pytest.raises(NotImplementedError):
            twin.rank_targets(f, qs)
