"""kg.MixedQuerySet and evaluation.eval_auc_queries / eval_perc_queries over {query type: MixedQuerySet}: queries of
DIFFERENT formulas scored window by window over a type's concatenation, and the models' score_ids_mixed behind it.

Without a GPU: the `tiny` index of tests/test_kg_sample.py on the host emulator of the kernels, all seven query types and
the scripted model of tests/test_eval_sets.py (score_ids only: the windows' runs are walked). On the GPU: both models on
the same graph -- score_ids_mixed against the concatenated score_ids bit for bit (the fused launch and, with fused =
False, the fallback), and both metrics against the QuerySet route."""
import numpy as np
import pytest
import torch

from mpqe_amd import evaluation, ops
from mpqe_amd.kg import MixedQuerySet, QuerySet
from oracle import ref_cpu
from tests.test_eval_sets import NEG_MAX, TYPES, Stub, _mean_bound, _stub_score, _windows, emu_sets  # noqa: F401
from tests.test_kg_sample import tiny               # noqa: F401  (the fixture)


def _several_per_type(sets):
    by_type = {}
    for f in sets:
        by_type.setdefault(f.query_type, []).append(f)
    return by_type


def test_from_sets_keeps_order_offsets_and_boundaries(emu_sets):
    lib, index, sets = emu_sets
    mixed = MixedQuerySet.from_sets(sets)
    by_type = _several_per_type(sets)
    assert list(mixed) == list(by_type) and set(mixed) == set(TYPES)
    assert any(len(fs) > 1 for fs in by_type.values())              # (several formulas of a type: something is mixed)
    for qt, ms in mixed.items():
        group = [sets[f] for f in by_type[qt]]
        assert ms.query_type == qt and ms.formulas == tuple(by_type[qt])
        assert len(ms) == sum(len(qs) for qs in group)
        np.testing.assert_array_equal(ms.bounds, np.concatenate([[0], np.cumsum([len(qs) for qs in group])]))
        np.testing.assert_array_equal(ms.formula_of.numpy(), ms.formula_of_host)
        for k, qs in enumerate(group):
            lo, hi = int(ms.bounds[k]), int(ms.bounds[k + 1])
            assert (ms.formula_of_host[lo:hi] == k).all()
            assert torch.equal(ms.targets[lo:hi], qs.targets) and torch.equal(ms.anchors[lo:hi], qs.anchors)
            for whole, part, hard in ((ms.neg, qs.neg, False), (ms.hard, qs.hard, True)):
                assert (whole is None) == (part is None)
                if whole is None:
                    assert ms.offsets_host(hard) is None
                    continue
                host = ms.offsets_host(hard)
                np.testing.assert_array_equal(host, whole[1].numpy())
                a, b = int(host[lo]), int(host[hi])
                assert torch.equal(whole[0][a:b], part[0]) and torch.equal(whole[1][lo:hi + 1] - a, part[1])
        assert int(ms.neg[1][-1]) == ms.neg[0].shape[0]
    with pytest.raises(TypeError):
        MixedQuerySet.from_sets({f: [] for f in sets})


def _expected_auc(mixed, seed, batch_size, hard=False):
    """the list path's arithmetic over the stub's scores, the negatives re-drawn by evaluation.auc_window_seed's rule with
    the Python restatement of the library's sampler (oracle/ref_cpu.py)"""
    labels, preds, per = [], [], {}
    for t, (qt, ms) in enumerate(mixed.items()):
        cand, off = ((ms.hard if hard else ms.neg)[k].numpy() for k in (0, 1))
        anchors, targets = ms.anchors.tolist(), ms.targets.tolist()
        pos, neg = [], []
        for w, (lo, hi) in enumerate(_windows(len(ms), batch_size)):
            negs, bad = ref_cpu.sample_negatives(cand, off, np.arange(lo, hi), hi - lo, evaluation.auc_window_seed(seed, t, w))
            assert not bad
            pos += [float(_stub_score(anchors[i], targets[i])) for i in range(lo, hi)]
            neg += [float(_stub_score(anchors[i], int(n))) for i, n in zip(range(lo, hi), negs)]
        for k, formula in enumerate(ms.formulas):
            lo, hi = int(ms.bounds[k]), int(ms.bounds[k + 1])
            per[formula] = evaluation.roc_auc([1] * (hi - lo) + [0] * (hi - lo), np.nan_to_num(pos[lo:hi] + neg[lo:hi]))
        labels += [1] * len(pos) + [0] * len(neg)
        preds += pos + neg
    return evaluation.roc_auc(labels, np.nan_to_num(preds)), per


def _percentiles_of(fn, monkeypatch):
    """fn() with every ops.eval_percentiles result recorded -> (fn's value, the per-query percentiles in call order)"""
    seen = []
    real = ops.eval_percentiles

    def spy(counts, offsets):
        out = real(counts, offsets)
        seen.append(out.cpu().numpy())
        return out
    monkeypatch.setattr(ops, 'eval_percentiles', spy)
    value = fn()
    monkeypatch.setattr(ops, 'eval_percentiles', real)
    return value, np.concatenate(seen)


def test_both_loops_on_mixed_sets(emu_sets, monkeypatch):
    lib, index, sets = emu_sets
    mixed = MixedQuerySet.from_sets(sets)

    def never(self):
        raise AssertionError('QuerySet.queries() was called: the device route builds no Query object')
    monkeypatch.setattr(QuerySet, 'queries', never)
    stub = Stub()
    auc, per = evaluation.eval_auc_queries(mixed, stub, batch_size=3, seed=3, lib=lib)
    want_auc, want_per = _expected_auc(mixed, 3, 3)
    assert set(per) == set(sets) and list(per) == [f for ms in mixed.values() for f in ms.formulas]
    assert auc == want_auc
    assert per == want_per
    assert len({round(v, 6) for v in per.values()}) > 1
    other, _ = evaluation.eval_auc_queries(mixed, stub, batch_size=3, seed=4, lib=lib)
    assert other == _expected_auc(mixed, 4, 3)[0] and other != auc          # the seed reaches the draws

    # every query's percentile is the QuerySet route's (the windows differ, the queries and their lists do not)
    by_sets, p_sets = _percentiles_of(lambda: evaluation.eval_perc_queries(sets, stub, batch_size=3, lib=lib), monkeypatch)
    by_mixed, p_mixed = _percentiles_of(lambda: evaluation.eval_perc_queries(mixed, stub, batch_size=3, lib=lib), monkeypatch)
    order = [f for ms in mixed.values() for f in ms.formulas]
    start = dict(zip(sets, np.concatenate([[0], np.cumsum([len(qs) for qs in sets.values()])])))
    regrouped = np.concatenate([p_sets[start[f]:start[f] + len(sets[f])] for f in order])
    np.testing.assert_array_equal(p_mixed.view(np.int64), regrouped.view(np.int64))
    assert isinstance(by_mixed, float) and abs(by_mixed - by_sets) <= 2 * _mean_bound(p_sets)
    assert abs(by_mixed - np.mean(p_sets)) <= _mean_bound(p_sets)
    index.check()


def test_hard_negatives_and_kinds_do_not_mix(emu_sets, monkeypatch):
    lib, index, sets = emu_sets
    mixed = MixedQuerySet.from_sets(sets)
    inter = {qt: ms for qt, ms in mixed.items() if 'inter' in qt}
    chain = {qt: ms for qt, ms in mixed.items() if qt == '2-chain'}
    assert inter and chain
    stub = Stub()
    auc, per = evaluation.eval_auc_queries(inter, stub, batch_size=4, hard_negatives=True, seed=1, lib=lib)
    want_auc, want_per = _expected_auc(inter, 1, 4, hard=True)
    assert auc == want_auc and per == want_per
    inter_sets = {f: qs for f, qs in sets.items() if 'inter' in f.query_type}
    a = evaluation.eval_perc_queries(inter, stub, batch_size=4, hard_negatives=True, lib=lib)
    _, p_sets = _percentiles_of(lambda: evaluation.eval_perc_queries(inter_sets, stub, batch_size=4, hard_negatives=True,
                                                                     lib=lib), monkeypatch)
    assert 0.0 <= a <= 100.0 and abs(a - np.mean(p_sets)) <= _mean_bound(p_sets)
    for fn in (evaluation.eval_auc_queries, evaluation.eval_perc_queries):
        with pytest.raises(Exception, match='Hard negative examples can only be used with intersection queries'):
            fn(chain, stub, batch_size=4, hard_negatives=True, lib=lib)
    f0, qs0 = next(iter(sets.items()))
    for other in ((f0, qs0), ('x', [])):
        with pytest.raises(TypeError):                                      # the three kinds do not mix
            evaluation.eval_auc_queries(dict(list(chain.items()) + [other]), stub, lib=lib)
        with pytest.raises(TypeError):
            evaluation.eval_perc_queries(dict(list(chain.items()) + [other]), stub, lib=lib)


# ------------------------------------------------------------------------------------------------- the GPU, both models
@pytest.fixture(scope='module')
def gpu_mixed(tiny):
    """both models on the tiny graph, and sets of all seven query types with several formulas a type"""
    from mpqe_amd import synthetic
    from mpqe_amd.data_utils import make_feature_modules
    from mpqe_amd.encoders import DirectEncoder
    from mpqe_amd.kg import KGIndex
    from mpqe_amd.model import QueryEncoderDecoder, RGCNEncoderDecoder
    from mpqe_amd.utils import get_intersection_decoder, get_metapath_decoder
    schema, adj, _, _ = tiny
    D = 16
    device = torch.device('cuda:0')
    torch.manual_seed(11)
    graph = synthetic.SchemaGraph(schema, D)
    graph.adj_lists = adj
    fm, node_maps = make_feature_modules(schema.ids, D, schema.num_entities)
    enc = DirectEncoder(None, fm, node_maps)
    rgcn = RGCNEncoderDecoder(graph, enc, readout='mp', num_layers=3, shared_layers=False, adaptive=True,
                              weight_decay=0).to(device)
    rgcn.fused = False
    dims = {m: D for m in schema.modes}
    gqe = QueryEncoderDecoder(graph, enc, get_metapath_decoder(graph, dims, 'bilinear'),
                              get_intersection_decoder(graph, dims, 'mean')).to(device)
    index = KGIndex.from_graph(graph, node_maps, device)
    sets = index.sample_query_sets(TYPES, 24, seed=3, neg_sample_max=NEG_MAX)
    assert {f.query_type for f in sets} == set(TYPES)
    return index, sets, MixedQuerySet.from_sets(sets), {'rgcn': rgcn, 'gqe': gqe}


def _concatenated_score_ids(model, ms, sets, lo, hi, host):
    """score_ids formula by formula over queries [lo, hi) of a type's concatenation, in forward()'s layout of the window"""
    a, b = int(host[lo]), int(host[hi])
    out = torch.empty(hi - lo + b - a, dtype=torch.float32, device=ms.targets.device)
    for k, formula in enumerate(ms.formulas):
        l, h = max(lo, int(ms.bounds[k])), min(hi, int(ms.bounds[k + 1]))
        if l >= h:
            continue
        x, y = int(host[l]), int(host[h])
        s = model.score_ids(formula, ms.anchors[l:h], ms.targets[l:h], neg=(ms.neg[0][x:y], ms.neg[1][l:h + 1] - x))
        out[l - lo:h - lo] = s[:h - l]
        out[hi - lo + x - a:hi - lo + y - a] = s[h - l:]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('fused', [True, False])
def test_score_ids_mixed_is_score_ids_bit_for_bit(gpu_mixed, fused):
    index, sets, mixed, models = gpu_mixed
    model = models['gqe']
    model.fused = fused
    try:
        several = 0
        for qt, ms in mixed.items():
            host = ms.offsets_host()
            several += len(ms.formulas) > 1
            for lo, hi in _windows(len(ms), 7) + [(0, len(ms))]:
                a, b = int(host[lo]), int(host[hi])
                got = model.score_ids_mixed(ms.formulas, ms.formula_of[lo:hi], ms.anchors[lo:hi], ms.targets[lo:hi],
                                            neg=(ms.neg[0][a:b], ms.neg[1][lo:hi + 1] - a))
                want = _concatenated_score_ids(model, ms, sets, lo, hi, host)
                assert got.is_cuda and got.dtype == torch.float32 and got.shape == want.shape
                assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (qt, lo, hi)
            kept = model.__dict__['_mixed'].get(id(ms.formulas))
            assert kept is not None and kept[1] is ms.formulas and (kept[2] is not None) == fused
            only = model.score_ids_mixed(ms.formulas, ms.formula_of[:9], ms.anchors[:9], ms.targets[:9])
            assert model.__dict__['_mixed'][id(ms.formulas)] is kept    # (the descriptor block is kept between calls)
            want = torch.cat([model.score_ids(ms.formulas[f], ms.anchors[l:h], ms.targets[l:h])
                              for f, l, h in _runs(ms.formula_of_host[:9])])
            assert torch.equal(only.view(torch.int32), want.view(torch.int32))
        assert several >= 3
        model._check()
        assert model._err is None or int(model._err.item()) == 0
    finally:
        model.fused = True


def _runs(fo):
    from mpqe_amd.model import formula_runs
    return formula_runs(fo)


@pytest.mark.gpu
@pytest.mark.parametrize('which', ['gqe', 'rgcn'])
def test_metrics_on_mixed_sets_agree_with_the_query_set_route(gpu_mixed, which, monkeypatch):
    from mpqe_amd.sampling import NegativeSampler
    index, sets, mixed, models = gpu_mixed
    model = models[which]

    def expected_auc(which_mixed, seed, hard):
        """evaluation.roc_auc on score_ids' scores for the negatives auc_window_seed's rule draws"""
        labels, preds, per = [], [], {}
        for t, (qt, ms) in enumerate(which_mixed.items()):
            sampler = NegativeSampler.from_csr(ms.neg, ms.hard, index.device)
            pos, neg = [], []
            for w, (lo, hi) in enumerate(_windows(len(ms), 7)):
                negs = sampler.sample(torch.arange(lo, hi), evaluation.auc_window_seed(seed, t, w), hard)
                for f, l, h in _runs(ms.formula_of_host[lo:hi]):
                    s = model.score_ids(ms.formulas[f], ms.anchors[lo + l:lo + h], ms.targets[lo + l:lo + h],
                                        neg=(negs[l:h], torch.arange(h - l + 1, device=index.device))).cpu().tolist()
                    pos += s[:h - l]
                    neg += s[h - l:]
            for k, formula in enumerate(ms.formulas):
                lo, hi = int(ms.bounds[k]), int(ms.bounds[k + 1])
                per[formula] = evaluation.roc_auc([1] * (hi - lo) + [0] * (hi - lo), np.nan_to_num(pos[lo:hi] + neg[lo:hi]))
            labels += [1] * len(pos) + [0] * len(neg)
            preds += pos + neg
        return evaluation.roc_auc(labels, np.nan_to_num(preds)), per

    auc, per = evaluation.eval_auc_queries(mixed, model, batch_size=7, seed=5)
    want_auc, want_per = expected_auc(mixed, 5, False)
    assert auc == want_auc and per == want_per
    by_sets, p_sets = _percentiles_of(lambda: evaluation.eval_perc_queries(sets, model, batch_size=7), monkeypatch)
    by_mixed, p_mixed = _percentiles_of(lambda: evaluation.eval_perc_queries(mixed, model, batch_size=7), monkeypatch)
    order = [f for ms in mixed.values() for f in ms.formulas]
    start = dict(zip(sets, np.concatenate([[0], np.cumsum([len(qs) for qs in sets.values()])])))
    regrouped = np.concatenate([p_sets[start[f]:start[f] + len(sets[f])] for f in order])
    np.testing.assert_array_equal(p_mixed.view(np.int64), regrouped.view(np.int64))
    assert abs(by_mixed - np.mean(p_sets)) <= _mean_bound(p_sets)

    inter = {qt: ms for qt, ms in mixed.items() if 'inter' in qt}
    auc, per = evaluation.eval_auc_queries(inter, model, batch_size=7, hard_negatives=True, seed=5)
    want_auc, want_per = expected_auc(inter, 5, True)
    assert auc == want_auc and per == want_per
    inter_sets = {f: qs for f, qs in sets.items() if 'inter' in f.query_type}
    by_sets, p_sets = _percentiles_of(lambda: evaluation.eval_perc_queries(inter_sets, model, batch_size=7,
                                                                           hard_negatives=True), monkeypatch)
    by_mixed = evaluation.eval_perc_queries(inter, model, batch_size=7, hard_negatives=True)
    assert abs(by_mixed - np.mean(p_sets)) <= _mean_bound(p_sets)
    index.check()
    model._check()
    assert model._err is None or int(model._err.item()) == 0
