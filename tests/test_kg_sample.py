"""Sampling on the KG index through its Python surface (mpqe_amd/kg.py: KGIndex.sample_queries, KGAnswers.sample_*_csr,
KGIndex.sample_query_sets, QuerySet): on a CPU-resident index on the host emulator of the kernels (KGIndex(lib=...), as
tests/test_kg_host.py) and, marked gpu, on the device. The sets are checked against tests/kg_oracle.py (Python sets)."""
import numpy as np
import pytest
import torch

from mpqe_amd import _capi, synthetic
from mpqe_amd.data_utils import make_feature_modules
from mpqe_amd.graph import Query, reverse_relation
from mpqe_amd.kg import KGIndex, QuerySet
from tests import kg_oracle

TYPES = list(_capi.QUERY_TYPE_IDS)
NEG_MAX = 5


@pytest.fixture(scope='module')
def tiny():
    """the `tiny` shape with a real adjacency, and the same graph minus a held-out edge set (both directions)"""
    schema = synthetic.make_schema(*synthetic.KG_SHAPES['tiny'], seed=5)
    adj = synthetic.make_adjacency(schema, degree=3, seed=5)
    _, node_maps = make_feature_modules(schema.ids, 8, schema.num_entities)
    rng = np.random.RandomState(9)
    train_adj = {r: {n: set(s) for n, s in lists.items()} for r, lists in adj.items()}
    for rel in adj:
        for n in sorted(adj[rel]):
            for d in sorted(adj[rel][n]):
                if rng.rand() < 0.15:
                    train_adj[rel][n].discard(d)
                    train_adj[reverse_relation(rel)][d].discard(n)
    return schema, adj, train_adj, node_maps


def _graph(schema, adj):
    graph = synthetic.SchemaGraph(schema, 8)
    graph.adj_lists = adj
    return graph


@pytest.fixture(scope='module', params=['emu', pytest.param('gpu', marks=pytest.mark.gpu)])
def indices(request, tiny):
    schema, adj, train_adj, node_maps = tiny
    if request.param == 'emu':
        from tests.kernel_backend import EmuBackend
        lib, device = EmuBackend().lib, 'cpu'
    else:
        lib, device = None, 'cuda:0'
    return (request.param, KGIndex.from_graph(_graph(schema, adj), node_maps, device, lib=lib),
            KGIndex.from_graph(_graph(schema, train_adj), node_maps, device, lib=lib))


def _flat_edges(query_graph):
    out = []
    for item in query_graph[1:]:
        out += [item] if not isinstance(item[0], tuple) else list(item)
    return out


def _check_sets(sets, schema, adj, per_type, train_adj=None):
    by_type = {}
    for formula, qs in sets.items():
        assert isinstance(qs, QuerySet) and len(qs) > 0
        qt = formula.query_type
        by_type[qt] = by_type.get(qt, 0) + len(qs)
        queries = qs.queries()
        assert len(queries) == len(qs) and qs.anchors.shape == (len(qs), len(formula.anchor_modes))
        assert (qs.hard is not None) == ('inter' in qt)
        full = set(int(x) for x in schema.ids[formula.target_mode])
        for q in queries:
            assert q.formula == formula
            for x, rel, y in _flat_edges(q.query_graph):
                assert y in adj[tuple(rel)][x], (q.query_graph,)                 # grounded: every edge is in the graph
            answers, hard = kg_oracle.query_sets(adj, formula, q.anchor_nodes)
            assert q.target_node in answers
            neg = q.neg_samples
            assert 0 < len(neg) <= NEG_MAX and len(set(neg)) == len(neg) and set(neg) <= full - answers
            assert len(neg) == min(NEG_MAX, len(full - answers))
            if 'inter' in qt:
                h = q.hard_neg_samples
                assert 0 < len(h) <= NEG_MAX and len(set(h)) == len(h) and set(h) <= hard
                assert len(h) == min(NEG_MAX, len(hard))
            else:
                assert q.hard_neg_samples is None
            if train_adj is not None:
                assert q.target_node not in kg_oracle.query_sets(train_adj, formula, q.anchor_nodes)[0]
            back = Query.deserialize(q.serialize(), keep_graph=True)
            assert back == q and back.query_graph == q.query_graph and sorted(back.neg_samples) == sorted(neg)
            assert (back.hard_neg_samples is None) == (q.hard_neg_samples is None)
    assert all(0 < n <= per_type for n in by_type.values())
    return by_type


def _same(a, b):
    return list(a) == list(b) and all(
        torch.equal(a[f].targets, b[f].targets) and torch.equal(a[f].anchors, b[f].anchors) and
        torch.equal(a[f].neg[0], b[f].neg[0]) and torch.equal(a[f].neg[1], b[f].neg[1]) for f in a)


def test_sample_query_sets(indices, tiny):
    """Every returned query's target answers it; every sampled negative is outside the answers, every hard negative in the
    union flavour minus the answers; no list is longer than neg_sample_max, none is empty where the type needs it;
    Query.serialize round-trips; the same seed gives the same sets, another seed others."""
    which, index, _ = indices
    schema, adj, _, _ = tiny
    sets = index.sample_query_sets(TYPES, 12, seed=3, neg_sample_max=NEG_MAX)
    by_type = _check_sets(sets, schema, adj, 12)
    assert set(by_type) == set(TYPES) and sum(by_type.values()) >= 6 * 12
    index.check()
    again = index.sample_query_sets(TYPES, 12, seed=3, neg_sample_max=NEG_MAX)
    other = index.sample_query_sets(TYPES, 12, seed=4, neg_sample_max=NEG_MAX)
    assert _same(sets, again) and not _same(sets, other)


def test_test_queries_are_not_answered_by_the_training_graph(indices, tiny):
    which, index, train_index = indices
    schema, adj, train_adj, _ = tiny
    sets = index.sample_query_sets(TYPES, 6, seed=11, neg_sample_max=NEG_MAX, train_index=train_index, max_rounds=12)
    by_type = _check_sets(sets, schema, adj, 6, train_adj=train_adj)
    assert len(by_type) >= 5
    index.check()
    train_index.check()


def test_negative_sampler_draws_from_the_sampled_lists(indices, tiny):
    """QuerySet.negative_sampler(): draws are members of the query's own list (a 1-chain draws from the whole mode). On the
    emulator the sampler's device lists go through mpqe_sample_negatives of the emulated library."""
    which, index, _ = indices
    schema = tiny[0]
    sets = index.sample_query_sets(['1-chain', '3-inter'], 10, seed=21, neg_sample_max=NEG_MAX)
    for formula, qs in sets.items():
        sampler = qs.negative_sampler()
        B = len(qs)
        assert sampler.n == B and (sampler.shared is not None) == (formula.query_type == '1-chain')
        idx = np.arange(B, dtype=np.int64)[::-1].copy()
        queries = qs.queries()
        for hard in ([False, True] if formula.query_type == '3-inter' else [False]):
            if which == 'gpu':
                got = sampler.sample(idx, 5, hard_negatives=hard).cpu().tolist()
                sampler.check()
            else:
                cand, off = sampler.hard if hard else sampler.neg
                out = torch.empty(B, dtype=torch.long)
                t_idx = torch.from_numpy(idx)
                if sampler.shared is not None:
                    st = index.lib.mpqe_sample_negatives(sampler.shared.data_ptr(), sampler.shared.shape[0], None, 0, None, B, 5,
                                                         out.data_ptr(), sampler.err.data_ptr(), None)
                else:
                    st = index.lib.mpqe_sample_negatives(cand.data_ptr(), cand.shape[0], off.data_ptr(), B, t_idx.data_ptr(), B, 5,
                                                         out.data_ptr(), sampler.err.data_ptr(), None)
                assert st == 0 and int(sampler.err.item()) == 0
                got = out.tolist()
            for i, g in zip(idx.tolist(), got):
                if formula.query_type == '1-chain':
                    assert g in set(int(x) for x in schema.ids[formula.target_mode])
                else:
                    assert g in (queries[i].hard_neg_samples if hard else queries[i].neg_samples)


def test_sampled_csr_equals_the_full_one_below_the_cap(indices, tiny):
    """KGAnswers.sample_negative_csr / sample_hard_csr: with k above every list they ARE negative_csr() / hard_csr()"""
    which, index, _ = indices
    schema, adj, _, _ = tiny
    rng = np.random.RandomState(2)
    formula = synthetic.sample_formula(schema, '2-inter', rng)
    queries = synthetic.sample_grounded_queries(schema, adj, formula, 6, rng)
    ans = index.answers(formula, queries, hard=True)
    for capped, full in ((ans.sample_negative_csr(1000, 1), ans.negative_csr()), (ans.sample_hard_csr(1000, 1), ans.hard_csr())):
        assert torch.equal(capped[0], full[0]) and torch.equal(capped[1], full[1])
    ids, off = ans.sample_negative_csr(3, 1)
    assert off.tolist() == [3 * i for i in range(7)] and ids.shape[0] == 18
    assert not torch.equal(ids, ans.sample_negative_csr(3, 2)[0])
    index.check()


def test_sample_queries_returns_records(indices):
    which, index, _ = indices
    rec = index.sample_queries('3-chain_inter', 300, seed=1)
    assert rec.shape == (300, 10) and rec.dtype == torch.int64 and rec.device.type == index.device.type
    assert torch.equal(rec, index.sample_queries(6, 300, seed=1)) and int(rec[:, 0].sum()) > 100
    assert index.sample_queries('2-chain', 0, seed=1).shape == (0, 10)
    index.check()


# ---------------------------------------------------------------------------------------------- the device, end to end
def _random_edges(schema, degree, seed):
    """{relation: (src ids, dst ids)} closed under inverse, as arrays: no Python adjacency"""
    rng = np.random.RandomState(seed)
    edges = {}
    for rel in schema.typed_relations():
        inv = reverse_relation(rel)
        if rel in edges or inv == rel:
            continue
        src = np.repeat(schema.ids[rel[0]], degree)
        dst = schema.ids[rel[2]][rng.randint(len(schema.ids[rel[2]]), size=src.shape[0])]
        edges[rel], edges[inv] = (src, dst), (dst, src)
    return edges


@pytest.mark.gpu
def test_query_sets_feed_the_model_and_the_ranking():
    """A from_edges index of the aifb shape (no Python adjacency anywhere): model.margin_loss on a QuerySet's queries and
    eval_rank_queries(known_answers=index) run, and the error words stay clean."""
    from mpqe_amd.encoders import DirectEncoder
    from mpqe_amd.evaluation import eval_rank_queries
    from mpqe_amd.model import RGCNEncoderDecoder
    device = torch.device('cuda:0')
    schema = synthetic.make_schema(*synthetic.KG_SHAPES['aifb'], seed=1)
    torch.manual_seed(1)
    graph = synthetic.SchemaGraph(schema, 64)
    graph.full_lists = {m: [int(v) for v in ids] for m, ids in graph.full_lists.items()}
    fm, node_maps = make_feature_modules(schema.ids, 64, schema.num_entities)
    model = RGCNEncoderDecoder(graph, DirectEncoder(None, fm, node_maps), readout='mp', num_layers=3, shared_layers=False,
                               adaptive=True, weight_decay=0).to(device)
    index = KGIndex.from_edges(schema, _random_edges(schema, 2, 3), node_maps, device)
    sets = index.sample_query_sets(['2-chain', '3-inter'], 24, seed=5, neg_sample_max=20)
    assert sum(len(qs) for qs in sets.values()) == 48
    test_queries = {}
    for formula, qs in sets.items():
        queries = qs.queries()
        test_queries[formula] = queries
        loss = model.margin_loss(formula, queries, hard_negatives='inter' in formula.query_type)
        assert torch.isfinite(loss).all()
        sampler = qs.negative_sampler()
        negs = sampler.sample(np.arange(len(qs)), 3)
        assert negs.shape[0] == len(qs)
        sampler.check()
    out = eval_rank_queries(test_queries, model.eval(), batch_size=16, known_answers=index)
    assert out['num_queries'] == 48 and 0 < out['mrr'] <= 1
    index.check()
