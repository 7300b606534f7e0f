"""The KG index at model level on the GPU, on the small synthetic KG of tests/test_answer_gpu.py: filtered ranking with
exclude = KGAnswers against exclude = the oracle's id lists (both models), eval_rank_queries with the index against the dict
of synthetic._answers sets, and NegativeSampler.from_csr over the index's lists. Untrained models: what is compared is the
exclusion, and ranks are integers -- every comparison is exact."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

from tests import kg_oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def small():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import train_synthetic
    from mpqe_amd import synthetic
    from mpqe_amd.kg import KGIndex
    args = argparse.Namespace(kg='small', embed_dim=64, batch_size=64, steps=0, lr=0.01, readout='mp', degree=2, formulas=1,
                              train_queries=1, test_queries=40, weight_scale=1.0, seed=0, oracle=False, eval_every=0,
                              decoder='bilinear', inter_decoder='mean')
    schema, graph, node_maps, gqe, train, test = train_synthetic.build_gqe(args, torch.device(DEV))
    _, _, _, rgcn, _, _ = train_synthetic.build(args, torch.device(DEV))
    adj = synthetic.make_adjacency(schema, degree=args.degree, seed=args.seed)
    graph.adj_lists = adj
    index = KGIndex.from_graph(graph, node_maps, DEV)
    by_edges = train_synthetic.kg_index(args, schema, node_maps, torch.device(DEV))
    tq = train_synthetic.test_dict(test)
    known = {q: synthetic._answers(adj, f, list(q.anchor_nodes))[0] for f in tq for q in tq[f]}
    return argparse.Namespace(schema=schema, adj=adj, index=index, by_edges=by_edges, tq=tq, known=known,
                              models={'gqe': gqe.eval(), 'rgcn': rgcn.to(DEV).eval()})


def test_answers_equal_the_oracle_on_the_device(small):
    """every test query: answers, hard and plain negatives as id sets; the index built from arrays gives the same words"""
    for f, qs in small.tq.items():
        ans = small.index.answers(f, qs, hard=True)
        other = small.by_edges.answers(f, qs, hard=True, global_bits=True)
        assert torch.equal(ans.bits, other.bits) and torch.equal(ans.hard_bits, other.hard_bits)
        assert torch.equal(ans.counts, other.counts)
        full = small.schema.ids[f.target_mode]
        want = [kg_oracle.negatives(small.adj, full, f, q.anchor_nodes) for q in qs]
        assert [set(l.tolist()) for l in ans.negative_lists()] == [w[0] for w in want], str(f)
        assert [set(l.tolist()) for l in ans.hard_lists()] == [w[1] for w in want], str(f)
        assert [set(l.tolist()) for l in ans.lists()] == [set(small.known[q]) for q in qs], str(f)
        assert all(q.target_node in l for q, l in zip(qs, ans.lists()))
    small.index.check()
    small.by_edges.check()


@pytest.mark.parametrize('which', ['gqe', 'rgcn'])
def test_rank_targets_with_the_index_equals_the_lists(small, which):
    model = small.models[which]
    some = False
    for f, qs in small.tq.items():
        lists = [sorted(small.known[q]) for q in qs]
        ans = small.index.answers(f, qs)
        by_lists = model.rank_targets(f, qs, exclude=lists)
        by_index = model.rank_targets(f, qs, exclude=ans)
        raw = model.rank_targets(f, qs)
        assert torch.equal(by_lists, by_index), str(f)
        some = some or not torch.equal(raw, by_lists)
        ids_l, sc_l = model.answer(f, qs, k=10, exclude=lists)
        ids_i, sc_i = model.answer(f, qs, k=10, exclude=ans)
        assert torch.equal(ids_l, ids_i) and torch.equal(sc_l, sc_i), str(f)
        for i, q in enumerate(qs):
            assert not set(ids_i[i].tolist()) & set(small.known[q])
    assert some, 'no exclusion changed any rank: the comparison shows nothing'
    with pytest.raises(ValueError):
        f, qs = next(iter(small.tq.items()))
        model.rank_targets(f, qs, exclude=small.index.answers(f, qs[:-1]))


@pytest.mark.parametrize('which', ['gqe', 'rgcn'])
def test_eval_rank_queries_with_the_index_equals_the_dict(small, which):
    from mpqe_amd import evaluation
    model = small.models[which]
    by_dict = evaluation.eval_rank_queries(small.tq, model, batch_size=32, ks=(1, 3, 10), known_answers=small.known)
    by_index = evaluation.eval_rank_queries(small.tq, model, batch_size=32, ks=(1, 3, 10), known_answers=small.index)
    assert by_dict == by_index
    raw = evaluation.eval_rank_queries(small.tq, model, batch_size=32, ks=(1, 3, 10))
    assert raw['mrr'] <= by_index['mrr'] and raw != by_index


def test_negative_sampler_from_csr_draws_what_the_oracle_allows(small):
    from mpqe_amd.sampling import NegativeSampler
    drawn_hard = 0
    for f, qs in small.tq.items():
        if 'inter' not in f.query_type:
            continue
        ans = small.index.answers(f, qs, hard=True)
        want = [kg_oracle.negatives(small.adj, small.schema.ids[f.target_mode], f, q.anchor_nodes) for q in qs]
        sampler = NegativeSampler.from_csr(ans.negative_csr(), ans.hard_csr(), DEV)
        has_hard = np.array([i for i, w in enumerate(want) if w[1]], dtype=np.int64)
        idx = np.arange(len(qs), dtype=np.int64)
        for seed in (1, 2, 3):
            neg = sampler.sample(idx, seed).cpu().tolist()
            assert all(x in want[i][0] for i, x in zip(idx, neg)), str(f)
            if has_hard.size:
                hard = sampler.sample(has_hard, seed, hard_negatives=True).cpu().tolist()
                assert all(x in want[i][1] for i, x in zip(has_hard, hard)), str(f)
                drawn_hard += len(hard)
        sampler.check()
        empty = np.array([i for i, w in enumerate(want) if not w[1]], dtype=np.int64)
        if empty.size:                      # a query without hard negatives: -1 and the flag, as for an empty Python list
            assert sampler.sample(empty[:1], 1, hard_negatives=True).cpu().tolist() == [-1]
            with pytest.raises(IndexError):
                sampler.check()
    assert drawn_hard > 0
