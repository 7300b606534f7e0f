"""KGIndex.sample_query_sets(batched=True) -- a cost per query type, not per formula (mpqe_amd/kg.py: answers_mixed,
KGAnswersMixed, records_of) -- against the per-formula route it stands beside, on a CPU-resident index on the host emulator
of the kernels and, marked gpu, on the device. Everything compared is integers and compared exactly."""
import hashlib

import numpy as np
import pytest
import torch

from mpqe_amd import _capi, evaluation
from mpqe_amd.kg import KGAnswersMixed, KGIndex
from tests import kg_oracle
from tests import kg_sample_oracle as oracle
from tests import test_kg_sample as S

tiny = S.tiny
indices = S.indices
TYPES = S.TYPES


def _same_queries(a, b):
    assert set(a) == set(b)
    for f in a:
        assert b[f].formula == f
        for x, y in ((a[f].targets, b[f].targets), (a[f].anchors, b[f].anchors), (a[f].variables, b[f].variables)):
            assert x.dtype == y.dtype and torch.equal(x, y), f
        assert (a[f].hard is None) == (b[f].hard is None)


def _pairs(qs):
    return [qs.neg] + ([] if qs.hard is None else [qs.hard])


@pytest.mark.parametrize('with_train', [False, True], ids=['plain', 'train_index'])
def test_batched_equals_the_per_formula_route(indices, tiny, with_train):
    """The same formulas, and per formula the same targets, anchors and variables in the same order. neg_sample_max above the
    entity count: every list is whole and ascending, so the negative and hard CSRs are identical too. neg_sample_max = 3:
    every list has min(3, c) distinct members of the query's full negative (hard) set and is the restated draw
    (tests/kg_sample_oracle.py) under the seed rule sample_query_sets states -- QuerySet.draw holds the seed and the
    position it used."""
    which, index, train_index = indices
    schema, adj, train_adj, node_maps = tiny
    kw = dict(train_index=train_index, max_rounds=12) if with_train else {}
    per_type = 6 if with_train else 12
    plain = index.sample_query_sets(TYPES, per_type, seed=11, neg_sample_max=1000, **kw)
    batched = index.sample_query_sets(TYPES, per_type, seed=11, neg_sample_max=1000, batched=True, **kw)
    assert len(plain) > 20
    _same_queries(plain, batched)
    for f in plain:
        for p, q in zip(_pairs(plain[f]), _pairs(batched[f])):
            assert torch.equal(p[0], q[0]) and torch.equal(p[1], q[1]), f
        for hard in (False, True):
            mirror = batched[f].offsets_host(hard)
            assert (mirror is None) == (batched[f].hard is None and hard)
            if mirror is not None:
                np.testing.assert_array_equal(mirror, (batched[f].hard if hard else batched[f].neg)[1].cpu().numpy())
    if with_train:
        for f, qs in batched.items():
            for q in qs.queries():
                assert q.target_node not in kg_oracle.query_sets(train_adj, f, q.anchor_nodes)[0]
    few = index.sample_query_sets(TYPES, per_type, seed=11, neg_sample_max=3, batched=True, **kw)
    _same_queries(plain, few)
    maps = node_maps.numpy() if torch.is_tensor(node_maps) else np.asarray(node_maps)
    drawn = 0
    for f, qs in few.items():
        seeds, pos = qs.draw
        row_ids = index.row_ids_host[f.target_mode]
        full = set(int(x) for x in schema.ids[f.target_mode])
        anchors = qs.anchors.cpu().tolist()
        for which_list, pair in enumerate(_pairs(qs)):
            ids, off = pair[0].cpu().numpy(), pair[1].cpu().numpy()
            for i in range(len(qs)):
                answers, hard = kg_oracle.query_sets(adj, f, anchors[i])
                members = sorted(int(maps[x]) for x in (hard if which_list else full - answers))
                mine = ids[off[i]:off[i + 1]].tolist()
                assert len(mine) == min(3, len(members)) == len(set(mine)) and set(mine) <= set(row_ids[members].tolist())
                want = oracle.sample_rows(members, 3, int(seeds[i]) + which_list, int(pos[i]))
                assert mine == row_ids[want].tolist(), (f, i)
                drawn += len(members) > 3
    assert drawn > 50
    index.check()
    train_index.check()


def _digest(sets):
    h = hashlib.sha256()
    for f in sorted(sets, key=lambda f: repr((f.query_type, f.rels))):
        qs = sets[f]
        h.update(repr((f.query_type, f.rels)).encode())
        for t in (qs.targets, qs.anchors, qs.variables, qs.neg[0], qs.neg[1]) + (tuple(qs.hard) if qs.hard else ()):
            h.update(np.ascontiguousarray(t.cpu().numpy()).tobytes())
    return h.hexdigest()


# what the commit before the batched route gives for sample_query_sets(TYPES, 12, seed=20261, neg_sample_max=5) on `tiny`:
# formulas, queries, the sum of the targets, the sum of the negatives, SHA-256 over every tensor of every set
PINNED = (69, 84, 2373, 11189, '8873427d1698040d25fdb723665e6f517fda6a988d704cb18f9700e0d3aaef29')


def test_default_route_is_unchanged(indices):
    which, index, _ = indices
    for kw in ({}, {'batched': False}):
        sets = index.sample_query_sets(TYPES, 12, seed=20261, neg_sample_max=5, **kw)
        got = (len(sets), sum(len(q) for q in sets.values()), int(sum(int(q.targets.sum()) for q in sets.values())),
               int(sum(int(q.neg[0].sum()) for q in sets.values())), _digest(sets))
        assert got == PINNED
    batched = index.sample_query_sets(TYPES, 12, seed=20261, neg_sample_max=5, batched=True)
    assert _digest(batched) != PINNED[4] and len(batched) == PINNED[0]          # (the draws below the cap differ, by the rule)
    again = index.sample_query_sets(TYPES, 12, seed=20261, neg_sample_max=5, batched=True)
    assert _digest(batched) == _digest(again)


class _Counting(object):
    """a bound library whose int-returning entry points are counted by name"""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in _capi.PROTOTYPES:
            return fn

        def counted(*args):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*args)
        return counted


def test_no_call_per_formula(tiny):
    """The library calls of one round of one type, counted through a wrapping lib: the same for 5 and for 50 kept queries
    -- about as many formulas on this schema -- under batched=True, while the per-formula route's grow with the formulas."""
    from tests.kernel_backend import EmuBackend
    schema, adj, _, node_maps = tiny
    lib = _Counting(EmuBackend().lib)
    index = KGIndex.from_graph(S._graph(schema, adj), node_maps, 'cpu', lib=lib)
    train = KGIndex.from_graph(S._graph(schema, tiny[2]), node_maps, 'cpu', lib=lib)
    index.table(), train.table()
    counts, formulas = {}, {}
    for batched in (True, False):
        for per_type in (5, 50):
            lib.calls = {}
            sets = index.sample_query_sets(['3-inter'], per_type, seed=2, neg_sample_max=4, train_index=train, max_rounds=1,
                                           batched=batched)
            assert sum(len(q) for q in sets.values()) == per_type
            counts[batched, per_type], formulas[batched, per_type] = dict(lib.calls), len(sets)
    assert formulas[True, 5] == formulas[False, 5] <= 5 and formulas[True, 50] == formulas[False, 50] >= 25
    assert counts[True, 5] == counts[True, 50]
    launches = {k: v for k, v in counts[True, 50].items() if not k.endswith('_bytes')}          # (size queries launch nothing)
    assert launches == {'mpqe_kg_sample_queries': 1, 'mpqe_kg_answers_mixed': 2, 'mpqe_kg_sample_rows_mixed': 2}
    assert sum(counts[False, 50].values()) > 4 * formulas[False, 50] > sum(counts[True, 50].values())


def test_batched_sets_feed_the_sampler_the_queries_and_the_auc(tiny):
    """downstream of a batched set, on the emulator: negative_sampler(), queries() (grounded, target an answer, negatives
    outside the answers) and eval_auc_queries over windows of the slices"""
    from tests.kernel_backend import EmuBackend
    from tests.test_eval_sets import Stub, _expected_auc
    schema, adj, _, node_maps = tiny
    lib = EmuBackend().lib
    index = KGIndex.from_graph(S._graph(schema, adj), node_maps, 'cpu', lib=lib)
    sets = index.sample_query_sets(TYPES, 10, seed=3, neg_sample_max=S.NEG_MAX, batched=True)
    by_type = S._check_sets(sets, schema, adj, 10)
    assert set(by_type) == set(TYPES)
    for formula, qs in sets.items():
        sampler = qs.negative_sampler()
        assert sampler.n == len(qs) and (sampler.shared is not None) == (formula.query_type == '1-chain')
        window = qs[1:3]
        assert len(window) == max(0, min(3, len(qs)) - 1) and window.offsets_host()[0] == 0
    auc, per = evaluation.eval_auc_queries(sets, Stub(), batch_size=3, seed=3, lib=lib)
    want_auc, want_per = _expected_auc(sets, 3, 3)
    assert auc == want_auc and per == want_per
    index.check()


# ---------------------------------------------------------------------------------------------- answers_mixed, records_of
def test_answers_mixed_of_listed_queries(indices, tiny):
    """records_of + answers_mixed on Query objects of several formulas of one type: lists() / hard_lists() are the oracle's
    sets, member says whether the target answers; a budget of one bitmap row chunks the batch and changes nothing, also
    not the sampled CSRs (the draw key takes the position in the whole batch)."""
    which, index, _ = indices
    schema, adj, _, _ = tiny
    sets = index.sample_query_sets(['3-inter_chain'], 20, seed=8, neg_sample_max=5)
    formulas, queries = [], []
    for f, qs in sets.items():
        for q in qs.queries():
            formulas.append(f)
            queries.append(q)
    assert len(set(formulas)) > 5
    records = index.records_of(formulas, queries)
    assert records.shape == (len(queries), _capi.KG_QUERY_INTS) and records.device.type == index.device.type
    whole = index.answers_mixed('3-inter_chain', records, hard=True)
    assert isinstance(whole, KGAnswersMixed) and whole.bits is not None and whole.hard_bits is not None
    for f, q, got, got_hard, member in zip(formulas, queries, whole.lists(), whole.hard_lists(), whole.member.cpu().tolist()):
        answers, hard = kg_oracle.query_sets(adj, f, q.anchor_nodes)
        assert set(got.tolist()) == answers and set(got_hard.tolist()) == hard and member == 1
    modes = [index.modes[m] for m in whole.target_mode.cpu().tolist()]
    assert modes == [f.target_mode for f in formulas] and len(set(modes)) > 1
    row_bytes = 4 * whole.W
    chunked = index.answers_mixed('3-inter_chain', records, hard=True, max_bitmap_bytes=2 * row_bytes * 3)
    bare = index.answers_mixed('3-inter_chain', records, hard=True, bits=False)
    for other in (chunked, bare):
        assert other.bits is None
        assert torch.equal(other.counts, whole.counts) and torch.equal(other.member, whole.member)
        assert torch.equal(other.target_mode, whole.target_mode)
    assert all(np.array_equal(a, b) for a, b in zip(chunked.lists(), whole.lists()))
    for k in (2, 1000):
        for a, b in ((whole.sample_negative_csr(k, 5), chunked.sample_negative_csr(k, 5)),
                     (whole.sample_hard_csr(k, 6), chunked.sample_hard_csr(k, 6))):
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[0].shape[0] > 0
    # probe rows: a row that is no answer
    probe = torch.full((len(queries),), -1, dtype=torch.int64)
    assert not index.answers_mixed('3-inter_chain', records, probe_rows=probe, bits=False).member.any()
    with pytest.raises(ValueError):
        index.answers_mixed('3-inter_chain', records).sample_hard_csr(3, 1)
    index.check()


def test_relation_the_training_index_lacks(tiny):
    """the KeyError of the per-formula route, from the batched one"""
    from mpqe_amd.graph import reverse_relation
    from tests.kernel_backend import EmuBackend
    schema, adj, train_adj, node_maps = tiny
    lib = EmuBackend().lib
    index = KGIndex.from_graph(S._graph(schema, adj), node_maps, 'cpu', lib=lib)
    gone = sorted(train_adj)[0]
    less = {r: l for r, l in train_adj.items() if r not in (gone, reverse_relation(gone))}
    train = KGIndex.from_graph(S._graph(schema, less), node_maps, 'cpu', lib=lib)
    for batched in (False, True):
        with pytest.raises(KeyError, match='no adjacency for relation'):
            index.sample_query_sets(['2-chain'], 40, seed=1, neg_sample_max=3, train_index=train, batched=batched)
    train.check()
