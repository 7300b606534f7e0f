"""evaluation.eval_rank_queries over {formula: kg.QuerySet} and {query type: kg.MixedQuerySet} (the device route), the
models' rank_ids / rank_ids_mixed behind it and KGIndex.records_of_ids.

Without a GPU: the `tiny` index of tests/test_kg_sample.py on the host emulator of the kernels, all seven query types, a
scripted model -- the windows, the answers from the device ids (index.answers, index.records_of_ids + index.answers_mixed),
the by-runs walk and the summary against the list route over QuerySet.queries(). On the GPU: both models on the `small`
synthetic KG (480 entities, 4 modes) -- rank_ids_mixed against rank_ids run by run, exactly, and the three routes'
dicts against each other. The models carry no drop-in, so the list route's rank_targets embeds on the module path as
rank_ids does: the routes rank the same embeddings and the dicts are equal, not close."""
import numpy as np
import pytest
import torch

from mpqe_amd import _capi, evaluation, synthetic
from mpqe_amd.data_utils import make_feature_modules
from mpqe_amd.kg import KGAnswers, KGIndex, MixedQuerySet
from mpqe_amd.model import formula_runs, rank_ids_by_runs
from tests.test_eval_sets import _stub_score
from tests.test_kg_sample import _graph, tiny               # noqa: F401  (the fixture)

TYPES = list(_capi.QUERY_TYPE_IDS)


def by_type(sets):
    """the dict's formulas grouped by query type, so that the list route meets them in MixedQuerySet.from_sets' order"""
    order = []
    for f in sets:
        if f.query_type not in order:
            order.append(f.query_type)
    return {f: qs for qt in order for f, qs in sets.items() if f.query_type == qt}


# ------------------------------------------------------------------------------------------ the emulator, a scripted model
class Stub(object):
    """rank_targets / rank_ids as a fixed function of the ids, on the host: every entity of the target mode scored by
    tests/test_eval_sets.py's _stub_score, ties to the smaller row, the answers taken from the KGAnswers' lists"""

    def __init__(self, index):
        self.index, self.calls = index, 0

    def _ranks(self, formula, anchors, targets, exclude):
        row_ids = self.index.row_ids_host[formula.target_mode]
        ids = row_ids[row_ids >= 0]
        assert exclude is None or (isinstance(exclude, KGAnswers) and len(exclude) == len(targets))
        known = [set()] * len(targets) if exclude is None else [set(int(x) for x in l) for l in exclude.lists()]
        out = []
        for a, t, ban in zip(anchors, targets, known):
            st = _stub_score(a, t)
            out.append(1 + sum(1 for c in ids.tolist() if c != t and c not in ban
                               and (_stub_score(a, c) > st or (_stub_score(a, c) == st and c < t))))
        return torch.tensor(out, dtype=torch.int64)

    def rank_targets(self, formula, queries, target_nodes=None, exclude=None):
        return self._ranks(formula, [list(q.anchor_nodes) for q in queries], list(target_nodes), exclude)

    def rank_ids(self, formula, anchors, targets, exclude=None, k=0):
        self.calls += 1
        return self._ranks(formula, anchors.tolist(), targets.tolist(), exclude), None, None


@pytest.fixture(scope='module')
def emu_world(tiny):
    from tests.kernel_backend import EmuBackend
    schema, adj, _, node_maps = tiny
    lib = EmuBackend().lib
    index = KGIndex.from_graph(_graph(schema, adj), node_maps, 'cpu', lib=lib)
    sets = by_type(index.sample_query_sets(TYPES, 10, seed=3, neg_sample_max=5))
    assert {f.query_type for f in sets} == set(TYPES)
    return index, sets, {f: qs.queries() for f, qs in sets.items()}, MixedQuerySet.from_sets(sets)


def test_records_of_ids_equals_records_of(emu_world):
    index, sets, lists, mixed = emu_world
    for qt, ms in mixed.items():
        formulas = [ms.formulas[f] for f in ms.formula_of_host]
        queries = [q for f in ms.formulas for q in lists[f]]
        want = index.records_of(formulas, queries)
        got = index.records_of_ids(ms.formulas, ms.formula_of, ms.anchors, ms.targets)
        assert got.dtype == torch.int64 and torch.equal(got, want), qt
        bare = index.records_of_ids(ms.formulas, ms.formula_of, ms.anchors)
        assert torch.equal(bare[:, 2:], want[:, 2:]) and (bare[:, 1] == -1).all()
        # an id that is no entity of its mode becomes the row past the mode's last; a formula out of range, no query
        fo, targets = ms.formula_of.clone(), ms.targets.clone()
        fo[0], targets[1] = len(ms.formulas), 10 ** 9
        odd = index.records_of_ids(ms.formulas, fo, ms.anchors, targets)
        assert (odd[0] == -1).all() and torch.equal(odd[2:], want[2:])
        mode = ms.formulas[int(ms.formula_of_host[1])].target_mode
        assert int(odd[1, 1]) == int(index.mode_rows[index.mode_index[mode]])


@pytest.mark.parametrize('filtered', [True, False])
def test_three_routes_give_one_dict_on_the_emulator(emu_world, filtered):
    index, sets, lists, mixed = emu_world
    stub = Stub(index)
    known = index if filtered else None
    want = evaluation.eval_rank_queries(lists, stub, batch_size=4, known_answers=known)
    assert want['num_queries'] == sum(len(qs) for qs in sets.values()) and set(want['per_formula']) == set(sets)
    got = evaluation.eval_rank_queries(sets, stub, batch_size=4, known_answers=known)
    assert got == want
    windows = sum(-(-len(qs) // 4) for qs in sets.values())
    assert stub.calls == windows
    stub.calls = 0
    got = evaluation.eval_rank_queries(mixed, stub, batch_size=4, known_answers=known)
    assert got == want
    runs = sum(len(formula_runs(ms.formula_of_host[lo:lo + 4])) for ms in mixed.values() for lo in range(0, len(ms), 4))
    assert stub.calls == runs                           # (a model without rank_ids_mixed: the windows' runs)
    if filtered:
        raw = evaluation.eval_rank_queries(sets, stub, batch_size=4)
        assert raw['mrr'] <= want['mrr'] and raw != want        # the filter takes entities out from before the target
    index.check()
    with pytest.raises(TypeError):
        evaluation.eval_rank_queries(sets, stub, known_answers={})


# ------------------------------------------------------------------------------------------------- the GPU, both models
D = 16
GPU_TYPES = ['1-chain', '2-chain', '2-inter', '3-inter', '3-inter_chain', '3-chain_inter']


def _models(graph, enc, schema, device, readout='mp'):
    from mpqe_amd.model import QueryEncoderDecoder, RGCNEncoderDecoder
    from mpqe_amd.utils import get_intersection_decoder, get_metapath_decoder
    rgcn = RGCNEncoderDecoder(graph, enc, readout=readout, num_layers=3, shared_layers=False, adaptive=True,
                              weight_decay=0).to(device).eval()
    dims = {m: D for m in schema.modes}
    gqe = QueryEncoderDecoder(graph, enc, get_metapath_decoder(graph, dims, 'bilinear'),
                              get_intersection_decoder(graph, dims, 'mean')).to(device).eval()
    return {'rgcn': rgcn, 'gqe': gqe}


@pytest.fixture(scope='module')
def gpu_world():
    """the `small` KG on the device: index, sets, their Query lists, the mixed sets and both models"""
    from mpqe_amd.encoders import DirectEncoder
    device = torch.device('cuda:0')
    schema = synthetic.make_schema(480, 4, 8, seed=0)
    adj = synthetic.make_adjacency(schema, degree=2, seed=0)
    torch.manual_seed(0)
    graph = synthetic.SchemaGraph(schema, D)
    graph.adj_lists = adj
    fm, node_maps = make_feature_modules(schema.ids, D, schema.num_entities)
    enc = DirectEncoder(None, fm, node_maps)
    models = _models(graph, enc, schema, device)
    models['rgcn_mlp'] = _models(graph, enc, schema, device, readout='mlp')['rgcn']
    index = KGIndex.from_graph(graph, node_maps, device)
    sets = by_type(index.sample_query_sets(GPU_TYPES, 40, seed=2, neg_sample_max=5))
    index.check()
    assert {f.query_type for f in sets} == set(GPU_TYPES)
    return index, sets, {f: qs.queries() for f, qs in sets.items()}, MixedQuerySet.from_sets(sets), models


@pytest.mark.gpu
@pytest.mark.parametrize('which', ['rgcn', 'gqe'])
def test_rank_ids_mixed_equals_rank_ids_by_runs(gpu_world, which):
    index, sets, lists, mixed, models = gpu_world
    model = models[which]
    k = 5
    took_mixed = 0
    assert any(len({f.target_mode for f in ms.formulas}) > 1 for ms in mixed.values()), 'no window mixes target modes'
    for qt, ms in mixed.items():
        for lo in range(0, len(ms), 32):
            hi = min(lo + 32, len(ms))
            fo, anchors, targets = ms.formula_of[lo:hi], ms.anchors[lo:hi], ms.targets[lo:hi]
            for filtered in (True, False):
                exclude = index.answers_mixed(qt, index.records_of_ids(ms.formulas, fo, anchors, targets)) if filtered else None
                ranks, ids, scores = model.rank_ids_mixed(ms.formulas, fo, anchors, targets, exclude, k)
                want = rank_ids_by_runs(model, ms.formulas, ms.formula_of_host[lo:hi], anchors, targets, exclude, k)
                assert ranks.dtype == torch.int64 and ranks.is_cuda and (ranks >= 1).all()
                assert torch.equal(ranks, want[0]), (which, qt, lo)
                assert torch.equal(ids, want[1]) and torch.equal(scores.view(torch.int32), want[2].view(torch.int32))
                if filtered:                            # the answers are not proposed
                    answers = exclude.lists()
                    assert all(not (set(ids[i].tolist()) & set(int(x) for x in answers[i])) for i in range(hi - lo))
        took_mixed += model._embed_mixed(ms.formulas, ms.formula_of[:1].to(model._device()),
                                         ms.anchors[:1].to(model._device())) is not None
    # (the mixed launch is what ran: every type for R-GCN, the four intersection types for GQE)
    assert took_mixed == (len(mixed) if which == 'rgcn' else sum('inter' in qt for qt in mixed))
    index.check()


@pytest.mark.gpu
@pytest.mark.parametrize('which', ['rgcn', 'gqe', 'rgcn_mlp'])
def test_three_routes_give_one_dict_on_the_gpu(gpu_world, which):
    """rgcn_mlp: a learned readout, which the mixed embedding does not cover -- rank_ids_mixed walks the runs. gqe: the
    chain types walk the runs too (their candidates are a projected table per formula)."""
    index, sets, lists, mixed, models = gpu_world
    model = models[which]
    if which == 'rgcn_mlp':
        ms = next(iter(mixed.values()))
        assert model._embed_mixed(ms.formulas, ms.formula_of[:1], ms.anchors[:1]) is None
    for known in (index, None):
        want = evaluation.eval_rank_queries(lists, model, batch_size=16, known_answers=known)
        assert want['num_queries'] == sum(len(qs) for qs in sets.values())
        assert evaluation.eval_rank_queries(sets, model, batch_size=16, known_answers=known) == want
        assert evaluation.eval_rank_queries(mixed, model, batch_size=16, known_answers=known) == want
    index.check()


@pytest.mark.gpu
def test_a_target_of_another_mode_raises(gpu_world):
    index, sets, lists, mixed, models = gpu_world
    model = models['rgcn']
    ms = mixed['2-inter']
    targets = ms.targets[:8].clone()
    other = next(m for m in index.modes if m != ms.formulas[int(ms.formula_of_host[3])].target_mode)
    targets[3] = int(index.row_ids_host[other][index.row_ids_host[other] >= 0][0])
    with pytest.raises(IndexError):
        model.rank_ids_mixed(ms.formulas, ms.formula_of[:8], ms.anchors[:8], targets)
    bits_free = index.answers_mixed('2-inter', index.records_of_ids(ms.formulas, ms.formula_of[:8], ms.anchors[:8]), bits=False)
    with pytest.raises(ValueError):
        model.rank_ids_mixed(ms.formulas, ms.formula_of[:8], ms.anchors[:8], ms.targets[:8], bits_free)
