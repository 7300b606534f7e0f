"""RGCNEncoderDecoder.score_ids_mixed and the device evaluation loops over {query type: kg.MixedQuerySet} on the GPU: the
R-GCN model's mixed launch (ops.rgcn_scores_mixed, csrc/rgcn_mixed.hip) against the concatenated score_ids BIT FOR BIT,
the launch count and host work of the loops, both metrics against the QuerySet route, the fallbacks and the kept
descriptor block. The model is tests/test_eval_mixed_sets.py's `gpu_mixed` R-GCN with fused = True."""
import numpy as np
import pytest
import torch

from mpqe_amd import evaluation, ops
from mpqe_amd.kg import MixedQuerySet, QuerySet
from tests.test_eval_mixed_sets import _concatenated_score_ids, _percentiles_of, _runs
from tests.test_eval_sets import NEG_MAX, TYPES, _mean_bound, _windows
from tests.test_kg_sample import tiny               # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

_BUILT = {}


def build(tiny, D=16, readout='mp'):  # noqa: F811
    """(index, sets, mixed, model) on the tiny graph: all seven query types, several formulas a type. Built once per
    (D, readout) and shared; a test that changes the model puts it back."""
    key = (D, readout)
    if key in _BUILT:
        return _BUILT[key]
    from mpqe_amd import synthetic
    from mpqe_amd.data_utils import make_feature_modules
    from mpqe_amd.encoders import DirectEncoder
    from mpqe_amd.kg import KGIndex
    from mpqe_amd.model import RGCNEncoderDecoder
    schema, adj, _, _ = tiny
    device = torch.device('cuda:0')
    torch.manual_seed(11)
    graph = synthetic.SchemaGraph(schema, D)
    graph.adj_lists = adj
    fm, node_maps = make_feature_modules(schema.ids, D, schema.num_entities)
    enc = DirectEncoder(None, fm, node_maps)
    model = RGCNEncoderDecoder(graph, enc, readout=readout, num_layers=3, shared_layers=False, adaptive=True,
                               weight_decay=0).to(device)
    assert model.fused
    index = KGIndex.from_graph(graph, node_maps, device)
    sets = index.sample_query_sets(TYPES, 24, seed=3, neg_sample_max=NEG_MAX)
    assert {f.query_type for f in sets} == set(TYPES)
    _BUILT[key] = (index, sets, MixedQuerySet.from_sets(sets), model)
    return _BUILT[key]


class Calls(object):
    """ops.rgcn_scores_mixed counted (one call = one mpqe_rgcn_fwd_mixed library call)"""

    def __init__(self, monkeypatch):
        self.n, real = 0, ops.rgcn_scores_mixed

        def spy(*args, **kwargs):
            self.n += 1
            return real(*args, **kwargs)
        monkeypatch.setattr(ops, 'rgcn_scores_mixed', spy)


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _check_bits(model, mixed, sets, windows=True):
    several = 0
    for qt, ms in mixed.items():
        host = ms.offsets_host()
        several += len(ms.formulas) > 1
        for lo, hi in (_windows(len(ms), 7) if windows else []) + [(0, len(ms))]:
            a, b = int(host[lo]), int(host[hi])
            got = model.score_ids_mixed(ms.formulas, ms.formula_of[lo:hi], ms.anchors[lo:hi], ms.targets[lo:hi],
                                        neg=(ms.neg[0][a:b], ms.neg[1][lo:hi + 1] - a))
            want = _concatenated_score_ids(model, ms, sets, lo, hi, host)
            assert got.is_cuda and got.dtype == torch.float32
            assert _bits_equal(got, want), (qt, lo, hi)
            assert torch.isfinite(want).all() and float(want.std()) > 0
        only = model.score_ids_mixed(ms.formulas, ms.formula_of[:9], ms.anchors[:9], ms.targets[:9])        # neg = None
        want = torch.cat([model.score_ids(ms.formulas[f], ms.anchors[l:h], ms.targets[l:h])
                          for f, l, h in _runs(ms.formula_of_host[:9])])
        assert _bits_equal(only, want)
    assert several >= 3
    model._check()
    assert model._err is None or int(model._err.item()) == 0


def test_score_ids_mixed_is_score_ids_bit_for_bit(tiny, monkeypatch):  # noqa: F811
    index, sets, mixed, model = build(tiny)
    calls = Calls(monkeypatch)
    _check_bits(model, mixed, sets)
    assert calls.n == sum(len(_windows(len(ms), 7)) + 2 for ms in mixed.values())
    for ms in mixed.values():
        kept = model.__dict__['_mixed'].get(id(ms.formulas))
        assert kept is not None and kept[1] is ms.formulas and kept[2] is not None


@pytest.mark.parametrize('D,readout', [(128, 'mp'), (16, 'sum'), (16, 'max'), (128, 'sum')])
def test_other_dims_and_readouts(tiny, monkeypatch, D, readout):  # noqa: F811
    index, sets, mixed, model = build(tiny, D, readout)
    calls = Calls(monkeypatch)
    _check_bits(model, mixed, sets, windows=False)
    assert calls.n == 2 * len(mixed)


def test_input_checks_are_the_gqe_model_s(tiny):  # noqa: F811
    index, sets, mixed, model = build(tiny)
    ms = mixed['2-inter']
    other = mixed['2-chain']
    with pytest.raises(TypeError):
        model.score_ids_mixed(ms.formulas, ms.formula_of.to(torch.int32), ms.anchors, ms.targets)
    with pytest.raises(ValueError):
        model.score_ids_mixed(ms.formulas, ms.formula_of[:3], ms.anchors, ms.targets)
    with pytest.raises(ValueError):
        model.score_ids_mixed(tuple(ms.formulas) + tuple(other.formulas), ms.formula_of, ms.anchors, ms.targets)
    with pytest.raises(ValueError):
        model.score_ids_mixed((), ms.formula_of, ms.anchors, ms.targets)
    bad = ms.formula_of.clone()
    bad[4] = len(ms.formulas)
    with pytest.raises(IndexError):
        model.score_ids_mixed(ms.formulas, bad, ms.anchors, ms.targets)
    assert int(model._err.item()) == 0          # (read and cleared)
    empty = model.score_ids_mixed(ms.formulas, ms.formula_of[:0], ms.anchors[:0], ms.targets[:0])
    assert empty.shape == (0,) and empty.dtype == torch.float32


def test_both_loops_make_one_library_call_per_window(tiny, monkeypatch):  # noqa: F811
    index, sets, mixed, model = build(tiny)

    def expected_auc(seed):
        """evaluation.roc_auc on score_ids' scores for the negatives auc_window_seed's rule draws"""
        from mpqe_amd.sampling import NegativeSampler
        labels, preds, per = [], [], {}
        for t, (qt, ms) in enumerate(mixed.items()):
            sampler = NegativeSampler.from_csr(ms.neg, ms.hard, index.device)
            pos, neg = [], []
            for w, (lo, hi) in enumerate(_windows(len(ms), 7)):
                negs = sampler.sample(torch.arange(lo, hi), evaluation.auc_window_seed(seed, t, w), False)
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

    # the QuerySet route and the expected AUC first: they go through score_ids
    want_auc, want_per = expected_auc(5)
    by_sets, p_sets = _percentiles_of(lambda: evaluation.eval_perc_queries(sets, model, batch_size=7), monkeypatch)

    def never(*args, **kwargs):
        raise AssertionError('the mixed route went through score_ids / QuerySet.queries')
    monkeypatch.setattr(type(model), 'score_ids', never)
    monkeypatch.setattr(QuerySet, 'queries', never)
    calls = Calls(monkeypatch)
    windows = sum(len(_windows(len(ms), 7)) for ms in mixed.values())
    auc, per = evaluation.eval_auc_queries(mixed, model, batch_size=7, seed=5)
    assert calls.n == windows
    assert auc == want_auc and per == want_per
    assert len({round(v, 6) for v in per.values()}) > 1
    by_mixed, p_mixed = _percentiles_of(lambda: evaluation.eval_perc_queries(mixed, model, batch_size=7), monkeypatch)
    assert calls.n == 2 * windows
    # every query's percentile equals the QuerySet route's to the bit
    order = [f for ms in mixed.values() for f in ms.formulas]
    start = dict(zip(sets, np.concatenate([[0], np.cumsum([len(qs) for qs in sets.values()])])))
    regrouped = np.concatenate([p_sets[start[f]:start[f] + len(sets[f])] for f in order])
    np.testing.assert_array_equal(p_mixed.view(np.int64), regrouped.view(np.int64))
    assert abs(by_mixed - np.mean(p_sets)) <= _mean_bound(p_sets)
    index.check()
    model._check()
    assert model._err is None or int(model._err.item()) == 0


@pytest.mark.parametrize('how', ['not_fused', 'mlp'])
def test_fallbacks_keep_the_layout_and_make_no_mixed_call(tiny, monkeypatch, how):  # noqa: F811
    index, sets, mixed, model = build(tiny) if how == 'not_fused' else build(tiny, 16, 'mlp')
    calls = Calls(monkeypatch)
    model.fused = how != 'not_fused'
    try:
        for qt in ('2-chain', '3-inter', '3-inter_chain'):
            ms = mixed[qt]
            host = ms.offsets_host()
            lo, hi = 3, len(ms) - 2
            a, b = int(host[lo]), int(host[hi])
            got = model.score_ids_mixed(ms.formulas, ms.formula_of[lo:hi], ms.anchors[lo:hi], ms.targets[lo:hi],
                                        neg=(ms.neg[0][a:b], ms.neg[1][lo:hi + 1] - a))
            want = _concatenated_score_ids(model, ms, sets, lo, hi, host)
            if how == 'not_fused':
                assert _bits_equal(got, want)
            else:
                # the learned readout sums a graph's (at most 4) node rows with fp32 atomics: score_ids itself differs
                # from call to call in the order of those additions. 3 re-ordered additions of O(1) terms are a few
                # ulp (1.2e-7 each) of the pooled row, which two Linear layers with O(1) weights over D = 16 inputs
                # and the cosine (a value in [-1, 1]) pass on at most ~D-fold: 2e-5 absolute. The LAYOUT is what this
                # checks: a score in another query's place is off by O(0.1).
                assert got.shape == want.shape and float((got - want).abs().max()) <= 2e-5
                assert float(want.std()) > 0.05
            kept = model.__dict__['_mixed'][id(ms.formulas)]
            assert kept[1] is ms.formulas and kept[2] is None
        assert calls.n == 0
    finally:
        model.fused = True


def test_descriptor_block_is_kept_and_rebuilt_when_a_table_moves(tiny, monkeypatch):  # noqa: F811
    from mpqe_amd import optim
    index, sets, mixed, model = build(tiny)
    ms = mixed['3-inter_chain']
    host = ms.offsets_host()

    def scores():
        got = model.score_ids_mixed(ms.formulas, ms.formula_of, ms.anchors, ms.targets, neg=ms.neg)
        assert _bits_equal(got, _concatenated_score_ids(model, ms, sets, 0, len(ms), host))
        return model.__dict__['_mixed'][id(ms.formulas)]

    built = []
    real = ops.RgcnMixedDescriptors

    def spy(*args, **kwargs):
        built.append(1)
        return real(*args, **kwargs)
    monkeypatch.setattr(ops, 'RgcnMixedDescriptors', spy)
    model.__dict__['_mixed'] = None
    first = scores()
    assert scores() is first and len(built) == 1                 # kept between calls
    # .to() round-trips the parameters: the kept blocks are dropped, the next call builds a new one
    model.to('cpu')
    assert model.__dict__['_mixed'] is None
    model.to('cuda:0')
    second = scores()
    assert second is not first and len(built) == 2
    # the flat optimiser re-homes every parameter (p.data becomes a view of one buffer): the addresses differ
    before = second[2].ptrs
    opt = optim.Adam([p for p in model.parameters() if p.requires_grad], lr=0.01)
    assert opt.flat
    assert tuple(model.enc.table(m).data_ptr() for m in second[3]) != before
    third = scores()
    assert third is not second and len(built) == 3 and third[2].ptrs != before
    assert scores() is third and len(built) == 3
    # copies and pickles drop the blocks
    import copy
    assert copy.deepcopy(model).__dict__['_mixed'] is None
