"""evaluation.eval_auc_queries / eval_perc_queries over {formula: kg.QuerySet} (the device route), and the models'
score_ids behind it.

Without a GPU: the `tiny` index of tests/test_kg_sample.py on the host emulator of the kernels, all seven query types, a
scripted model -- the two loops, the windows, the seed rule of the sampled negatives and the two metric kernels against the
list-path functions of evaluation.py. On the GPU: both models on the same graph -- score_ids against forward() on the same
ids bit for bit, and both metrics against the list-path functions fed forward()'s scores."""
import numpy as np
import pytest
import torch

from mpqe_amd import _capi, evaluation, synthetic
from mpqe_amd.data_utils import make_feature_modules
from mpqe_amd.kg import KGIndex, QuerySet
from oracle import ref_cpu
from tests.test_kg_sample import _graph, tiny               # noqa: F401  (the fixture)

TYPES = list(_capi.QUERY_TYPE_IDS)
NEG_MAX = 5


def _mean_bound(values):
    """a float64 sum of Q non-negative terms taken in another order: within Q 2^-52 relative"""
    return len(values) * 2.0 ** -52 * float(np.mean(values))


# ------------------------------------------------------------------------------------------ the emulator, a scripted model
def _stub_score(anchors, candidate):
    h = ref_cpu._mix64(candidate * 1000003 + sum((k + 1) * 7919 * int(a) for k, a in enumerate(anchors)))
    return np.float32((h % 201 - 100) / 100.0)              # two decimals in [-1, 1]: ties occur


class Stub(object):
    """score_ids as a fixed function of the ids, a CPU tensor in forward()'s layout"""

    def __init__(self):
        self.calls = 0

    def score_ids(self, formula, anchors, targets, neg=None):
        self.calls += 1
        a, t = anchors.tolist(), targets.tolist()
        assert len(a) == len(t) and all(len(row) == len(formula.anchor_modes) for row in a)
        ids, off = (x.tolist() for x in neg)
        assert len(off) == len(t) + 1 and off[0] == 0 and off[-1] == len(ids)
        rows = list(range(len(t))) + [i for i in range(len(t)) for _ in range(off[i + 1] - off[i])]
        return torch.from_numpy(np.array([_stub_score(a[r], c) for r, c in zip(rows, t + ids)], dtype=np.float32))


@pytest.fixture(scope='module')
def emu_sets(tiny):
    from tests.kernel_backend import EmuBackend
    schema, adj, _, node_maps = tiny
    lib = EmuBackend().lib
    index = KGIndex.from_graph(_graph(schema, adj), node_maps, 'cpu', lib=lib)
    sets = index.sample_query_sets(TYPES, 10, seed=3, neg_sample_max=NEG_MAX)
    assert {f.query_type for f in sets} == set(TYPES)
    return lib, index, sets


def _windows(n, batch_size):
    return [(lo, min(lo + batch_size, n)) for lo in range(0, n, batch_size)]


def _expected_auc(sets, seed, batch_size, hard=False):
    """the list path's arithmetic over the stub's scores, the negatives re-drawn by evaluation.auc_batch_seed's rule with
    the Python restatement of the library's sampler (oracle/ref_cpu.py)"""
    labels, preds, per = [], [], {}
    for f, (formula, qs) in enumerate(sets.items()):
        cand, off = ((qs.hard if hard else qs.neg)[k].numpy() for k in (0, 1))
        anchors, targets = qs.anchors.tolist(), qs.targets.tolist()
        f_labels, f_preds = [], []
        for b, (lo, hi) in enumerate(_windows(len(qs), batch_size)):
            negs, bad = ref_cpu.sample_negatives(cand, off, np.arange(lo, hi), hi - lo, evaluation.auc_batch_seed(seed, f, b))
            assert not bad
            f_labels += [1] * (hi - lo) + [0] * (hi - lo)
            f_preds += [float(_stub_score(anchors[i], targets[i])) for i in range(lo, hi)]
            f_preds += [float(_stub_score(anchors[i], int(n))) for i, n in zip(range(lo, hi), negs)]
        per[formula] = evaluation.roc_auc(f_labels, np.nan_to_num(f_preds))
        labels += f_labels
        preds += f_preds
    return evaluation.roc_auc(labels, np.nan_to_num(preds)), per


def test_both_loops_on_query_sets_without_a_host_list(emu_sets, monkeypatch):
    lib, index, sets = emu_sets

    def never(self):
        raise AssertionError('QuerySet.queries() was called: the device route builds no Query object')
    monkeypatch.setattr(QuerySet, 'queries', never)
    stub = Stub()
    auc, per = evaluation.eval_auc_queries(sets, stub, batch_size=3, seed=3, lib=lib)
    want_auc, want_per = _expected_auc(sets, 3, 3)
    assert list(per) == list(sets) and stub.calls == sum(len(_windows(len(qs), 3)) for qs in sets.values())
    assert auc == want_auc
    assert per == want_per
    assert len({round(v, 6) for v in per.values()}) > 1                     # (not all 0.5: the scores do differ)
    other, _ = evaluation.eval_auc_queries(sets, stub, batch_size=3, seed=4, lib=lib)
    assert other == _expected_auc(sets, 4, 3)[0] and other != auc           # the seed reaches the draws

    perc = evaluation.eval_perc_queries(sets, stub, batch_size=3, lib=lib)
    want = []
    for formula, qs in sets.items():
        ids, off = qs.neg[0].tolist(), qs.neg[1].tolist()
        anchors, targets = qs.anchors.tolist(), qs.targets.tolist()
        for i in range(len(qs)):
            negs = [float(_stub_score(anchors[i], n)) for n in ids[off[i]:off[i + 1]]]
            want.append(evaluation.percentile_of_score(negs, float(_stub_score(anchors[i], targets[i]))))
    assert isinstance(perc, float) and abs(perc - np.mean(want)) <= _mean_bound(want)
    index.check()


def test_hard_negatives_on_query_sets(emu_sets):
    lib, index, sets = emu_sets
    inter = {f: qs for f, qs in sets.items() if 'inter' in f.query_type}
    chain = {f: qs for f, qs in sets.items() if f.query_type == '2-chain'}
    assert inter and chain
    stub = Stub()
    auc, per = evaluation.eval_auc_queries(inter, stub, batch_size=4, hard_negatives=True, seed=1, lib=lib)
    want_auc, want_per = _expected_auc(inter, 1, 4, hard=True)
    assert auc == want_auc and per == want_per
    assert 0.0 <= evaluation.eval_perc_queries(inter, stub, batch_size=4, hard_negatives=True, lib=lib) <= 100.0
    for fn in (evaluation.eval_auc_queries, evaluation.eval_perc_queries):
        with pytest.raises(Exception, match='Hard negative examples can only be used with intersection queries'):
            fn(chain, stub, batch_size=4, hard_negatives=True, lib=lib)
    with pytest.raises(TypeError):                                          # sets and lists do not mix
        evaluation.eval_auc_queries(dict(list(chain.items()) + [('x', [])]), stub, lib=lib)


def test_query_set_windows(emu_sets):
    """QuerySet[lo:hi]: the same queries, CSRs re-based to 0"""
    lib, index, sets = emu_sets
    for formula, qs in sets.items():
        whole = qs.queries()
        n = len(qs)
        for lo, hi in [(0, n), (1, n), (0, 1), (n // 2, n // 2), (1, min(4, n)), (n - 1, n + 5)]:
            part = qs[lo:hi]
            assert isinstance(part, QuerySet) and len(part) == len(whole[lo:hi]) and part.formula == formula
            assert int(part.neg[1][0]) == 0 and int(part.neg[1][-1]) == part.neg[0].shape[0]
            np.testing.assert_array_equal(part.offsets_host(), part.neg[1].numpy())
            got = part.queries()
            assert got == whole[lo:hi]
            assert [q.neg_samples for q in got] == [q.neg_samples for q in whole[lo:hi]]
            assert [q.hard_neg_samples for q in got] == [q.hard_neg_samples for q in whole[lo:hi]]
        with pytest.raises(TypeError):
            qs[0]
        with pytest.raises(TypeError):
            qs[::2]


# ------------------------------------------------------------------------------------------------- the GPU, both models
GPU_TYPES = ['2-chain', '3-inter', '3-inter_chain']
D = 16


@pytest.fixture(scope='module')
def gpu_world(tiny):
    """the device index, its sets with their Query lists, and both models on the tiny graph"""
    from mpqe_amd.encoders import DirectEncoder
    from mpqe_amd.model import QueryEncoderDecoder, RGCNEncoderDecoder
    from mpqe_amd.utils import get_intersection_decoder, get_metapath_decoder
    schema, adj, _, _ = tiny
    device = torch.device('cuda:0')
    torch.manual_seed(11)
    graph = synthetic.SchemaGraph(schema, D)
    graph.adj_lists = adj
    fm, node_maps = make_feature_modules(schema.ids, D, schema.num_entities)
    enc = DirectEncoder(None, fm, node_maps)
    rgcn = RGCNEncoderDecoder(graph, enc, readout='mp', num_layers=3, shared_layers=False, adaptive=True,
                              weight_decay=0).to(device)
    rgcn.fused = False                      # the comparison side: forward() on the module path
    dims = {m: D for m in schema.modes}
    gqe = QueryEncoderDecoder(graph, enc, get_metapath_decoder(graph, dims, 'bilinear'),
                              get_intersection_decoder(graph, dims, 'mean')).to(device)
    index = KGIndex.from_graph(graph, node_maps, device)
    sets = index.sample_query_sets(GPU_TYPES, 24, seed=3, neg_sample_max=NEG_MAX)
    assert {f.query_type for f in sets} == set(GPU_TYPES)
    lists = {f: qs.queries() for f, qs in sets.items()}
    return index, sets, lists, {'rgcn': rgcn, 'gqe': gqe}


def _forward_all(model, formula, queries, lo, hi, pool):
    lengths = [len(getattr(q, pool)) for q in queries[lo:hi]]
    negatives = [n for q in queries[lo:hi] for n in getattr(q, pool)]
    with torch.no_grad():
        return model.forward(formula, queries[lo:hi], [q.target_node for q in queries[lo:hi]], neg_nodes=negatives,
                             neg_lengths=lengths), lengths


@pytest.mark.gpu
@pytest.mark.parametrize('which', ['gqe', 'rgcn'])
def test_score_ids_is_forward_bit_for_bit(gpu_world, which):
    index, sets, lists, models = gpu_world
    model = models[which]
    for formula, qs in sets.items():
        host = qs.offsets_host()
        for lo, hi in _windows(len(qs), 7):
            a, b = int(host[lo]), int(host[hi])
            got = model.score_ids(formula, qs.anchors[lo:hi], qs.targets[lo:hi], neg=(qs.neg[0][a:b], qs.neg[1][lo:hi + 1] - a))
            want, lengths = _forward_all(model, formula, lists[formula], lo, hi, 'neg_samples')
            assert got.is_cuda and got.dtype == torch.float32 and got.shape == want.shape == (hi - lo + sum(lengths),)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (which, formula, lo)
        only = model.score_ids(formula, qs.anchors[:7], qs.targets[:7])             # no negatives: the targets' scores alone
        with torch.no_grad():
            want = model.forward(formula, lists[formula][:7], [q.target_node for q in lists[formula][:7]])
        assert torch.equal(only.view(torch.int32), want.view(torch.int32))
    model._check()
    assert model._err is None or int(model._err.item()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize('which', ['gqe', 'rgcn'])
def test_metrics_on_sets_equal_the_list_path_on_the_same_scores(gpu_world, which, monkeypatch):
    from mpqe_amd.sampling import NegativeSampler
    index, sets, lists, models = gpu_world
    model = models[which]
    inter = {f: qs for f, qs in sets.items() if 'inter' in f.query_type}
    chain = {f: qs for f, qs in sets.items() if f.query_type == '2-chain'}

    def never(self):
        raise AssertionError('QuerySet.queries() was called')
    monkeypatch.setattr(QuerySet, 'queries', never)

    def list_auc(which_sets, seed, hard):
        """eval_auc_queries' list-path arithmetic on forward()'s scores for the negatives the seed rule draws"""
        labels, preds, per = [], [], {}
        for f, (formula, qs) in enumerate(which_sets.items()):
            sampler = NegativeSampler.from_csr(qs.neg, qs.hard, index.device)
            f_labels, f_preds = [], []
            for b, (lo, hi) in enumerate(_windows(len(qs), 7)):
                negs = sampler.sample(torch.arange(lo, hi), evaluation.auc_batch_seed(seed, f, b), hard).cpu().tolist()
                queries = lists[formula][lo:hi]
                with torch.no_grad():
                    scores = model.forward(formula, queries, [q.target_node for q in queries], neg_nodes=negs,
                                           neg_lengths=[1] * (hi - lo))
                f_labels += [1] * (hi - lo) + [0] * (hi - lo)
                f_preds += scores.cpu().tolist()
            per[formula] = evaluation.roc_auc(f_labels, np.nan_to_num(f_preds))
            labels += f_labels
            preds += f_preds
        return evaluation.roc_auc(labels, np.nan_to_num(preds)), per

    def list_perc(which_sets, pool):
        out = []
        for formula, qs in which_sets.items():
            for lo, hi in _windows(len(qs), 7):
                scores, lengths = _forward_all(model, formula, lists[formula], lo, hi, pool)
                out += evaluation._get_perc_scores(scores.cpu().tolist(), lengths)
        return out

    auc, per = evaluation.eval_auc_queries(sets, model, batch_size=7, seed=5)
    want_auc, want_per = list_auc(sets, 5, False)
    assert auc == want_auc and per == want_per
    perc = evaluation.eval_perc_queries(sets, model, batch_size=7)
    want = list_perc(sets, 'neg_samples')
    assert abs(perc - np.mean(want)) <= _mean_bound(want)

    auc, per = evaluation.eval_auc_queries(inter, model, batch_size=7, hard_negatives=True, seed=5)
    want_auc, want_per = list_auc(inter, 5, True)
    assert auc == want_auc and per == want_per
    perc = evaluation.eval_perc_queries(inter, model, batch_size=7, hard_negatives=True)
    want = list_perc(inter, 'hard_neg_samples')
    assert abs(perc - np.mean(want)) <= _mean_bound(want)
    for fn in (evaluation.eval_auc_queries, evaluation.eval_perc_queries):
        with pytest.raises(Exception, match='Hard negative examples can only be used with intersection queries'):
            fn(chain, model, batch_size=7, hard_negatives=True)
    index.check()
    model._check()
    assert model._err is None or int(model._err.item()) == 0
