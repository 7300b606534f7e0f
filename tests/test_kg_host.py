"""Exact answers on the knowledge graph, the parts that need no GPU: the set oracle (tests/kg_oracle.py) against sets the
reference itself produced (tests/golden/kg_sets_small.npz, tools/gen_kg_golden.py), KGIndex's CSR construction against the
adjacency dicts, the entry points' argument checks on made-up device addresses, and the Python surface end to end with a
CPU-resident index on the host emulator of the kernels. Every comparison is exact: these are sets of integers."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from mpqe_amd import _capi, synthetic
from mpqe_amd.data_utils import make_feature_modules
from mpqe_amd.graph import Query
from mpqe_amd.kg import KGIndex, kg_programme
from tests import kg_oracle

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'kg_sets_small.npz')


# ---------------------------------------------------------------------------------------------- the oracle vs the reference
def _golden():
    z = np.load(GOLDEN)
    info = json.loads(bytes(z['meta']).decode())
    sch = info['schema']
    typed = [(m, name, to) for m in sch['modes'] for to, name in sch['relations'][m]]
    adj = {r: {int(n): set() for n in sch['ids'][r[0]]} for r in typed}
    for r, s, d in zip(z['adj_rel'], z['adj_src'], z['adj_dst']):
        adj[typed[int(r)]][int(s)].add(int(d))
    cases = []
    for c in range(len(z['types'])):
        qt = info['query_types'][int(z['types'][c])]
        edges = [(int(x), typed[int(r)], int(y)) for x, r, y in z['edges'][c] if r >= 0]
        graph = (qt,) + tuple(edges) if qt.endswith('-chain') or qt.endswith('-inter') else (qt, edges[0], (edges[1], edges[2]))

        def seg(name):
            return set(int(x) for x in z[name + '_ids'][z[name + '_off'][c]:z[name + '_off'][c + 1]])
        cases.append((Query(graph, keep_graph=True), bool(z['none'][c]), seg('neg'), seg('hard'), seg('meta')))
    return info, adj, cases


def test_fixture_is_small_and_covers_the_types():
    info, adj, cases = _golden()
    assert os.path.getsize(GOLDEN) < 100 * 1024
    types = [q.formula.query_type for q, _, _, _, _ in cases]
    assert set(types) == set(info['query_types']) and len(cases) >= 18
    assert any(none for _, none, _, _, _ in cases) and any(hard for _, _, _, hard, _ in cases)


def test_oracle_equals_the_reference_sets():
    """Graph.get_negative_samples returned (negatives, hard negatives) -- hard None for the chain types -- or (None, None)
    when one of the two sets is empty; Graph.get_metapath_neighs the answers of a chain."""
    info, adj, cases = _golden()
    ids = info['schema']['ids']
    for q, none, neg, hard, meta in cases:
        f = q.formula
        my_neg, my_hard = kg_oracle.negatives(adj, ids[f.target_mode], f, q.anchor_nodes)
        ans, _ = kg_oracle.query_sets(adj, f, q.anchor_nodes)
        chain = f.query_type.endswith('-chain')
        if none:
            assert not my_neg or (not chain and not my_hard), str(f)
        else:
            assert my_neg == neg, str(f)
            assert (my_hard == hard) if not chain else (not my_hard and not hard), str(f)
        if chain:
            assert ans == meta, str(f)
        assert ans == synthetic._answers(adj, f, list(q.anchor_nodes))[0], str(f)


# ---------------------------------------------------------------------------------------------- the index
@pytest.fixture(scope='module')
def tiny():
    schema = synthetic.make_schema(*synthetic.KG_SHAPES['tiny'], seed=5)
    adj = synthetic.make_adjacency(schema, degree=3, seed=5)
    _, node_maps = make_feature_modules(schema.ids, 8, schema.num_entities)
    graph = synthetic.SchemaGraph(schema, 8)
    graph.adj_lists = adj
    return schema, adj, node_maps, graph


def _edge_arrays(adj):
    out = {}
    for rel, lists in adj.items():
        src = [n for n, s in lists.items() for _ in s]
        dst = [d for s in lists.values() for d in s]
        out[rel] = (np.array(src, dtype=np.int64), np.array(dst, dtype=np.int64))
    return out


def test_index_csr_equals_the_adjacency(tiny):
    schema, adj, node_maps, graph = tiny
    a = KGIndex.from_graph(graph, node_maps, 'cpu')
    b = KGIndex.from_edges(schema, _edge_arrays(adj), node_maps, 'cpu')
    maps = node_maps.numpy()
    for index in (a, b):
        assert index.modes == schema.modes and set(index.rels) == set(adj)
        for m in schema.modes:
            n = index.row_ids_host[m].shape[0]
            assert n == len(schema.ids[m]) == int(index.mode_rows[index.mode_index[m]])
            np.testing.assert_array_equal(index.row_ids_host[m], schema.ids[m])
            valid = index.valid[m].numpy().view(np.uint32)
            assert valid.shape[0] == (n + 31) // 32
            assert [int(valid[r // 32] >> (r % 32)) & 1 for r in range(valid.shape[0] * 32)] == [1] * n + [0] * (valid.shape[0] * 32 - n)
        for rel in adj:
            i = index.rel_index[rel]
            off, rows = index.offsets[i].numpy(), index.rows[i].numpy()
            assert off.shape[0] == len(schema.ids[rel[0]]) + 1 and off[0] == 0 and off[-1] == rows.shape[0]
            assert rows.shape[0] == sum(len(s) for s in adj[rel].values())
            for node, neigh in adj[rel].items():
                r = maps[node]
                got = index.row_ids_host[rel[2]][rows[off[r]:off[r + 1]]]
                assert sorted(got.tolist()) == sorted(neigh), (rel, node)


def test_index_with_table_holes_and_bad_edges(tiny):
    """ids with gaps in their rows: n = 1 + the last row that is an entity, the rows between are no entities; an edge whose
    endpoint is of another mode is refused when the index is built."""
    node_maps = np.full(40, -1, dtype=np.int64)
    ids = {'a': np.array([3, 5, 9]), 'b': np.array([1, 2])}
    node_maps[[3, 5, 9]] = [0, 2, 5]
    node_maps[[1, 2]] = [1, 0]
    index = KGIndex.from_edges(ids, {('a', 'r', 'b'): ([3, 9, 9], [1, 2, 1])}, node_maps, 'cpu')
    assert index.mode_rows.tolist() == [6, 2] and index.num_entities == {'a': 3, 'b': 2}
    assert index.valid['a'].numpy().view(np.uint32).tolist() == [0b100101]
    assert index.offsets[0].tolist() == [0, 1, 1, 1, 1, 1, 3] and sorted(index.rows[0].tolist()[1:]) == [0, 1]
    with pytest.raises(IndexError):
        KGIndex.from_edges(ids, {('a', 'r', 'b'): ([3], [5])}, node_maps, 'cpu')
    with pytest.raises(RuntimeError, match='no CPU path'):
        index.answers(synthetic.Formula('1-chain', (('b', 'r', 'a'),)), np.array([[3]]))


# ---------------------------------------------------------------------------------------------- argument checks, no launch
def _libs():
    from mpqe_amd import _lib
    from tests.kernel_backend import EmuBackend
    return [('emu', EmuBackend().lib), ('product', _lib.load())]


@pytest.mark.parametrize('which', ['emu', 'product'])
def test_entry_points_refuse_before_any_launch(which):
    """Device pointers are made-up addresses: a call that launched anything with them would fault. Every call here must
    answer from its checks."""
    lib = dict(_libs())[which]
    fake = 0x10000
    # modes 0, 1 (40 and 100 000 rows: LDS and beyond it); relation 0: 0 -> 1, relation 1: 1 -> 0, relation 2: 0 -> 0
    prog = np.ascontiguousarray(kg_programme([(0, [(2, 0)]), (1, [(1, 0)])], [(2, 0)], 0))
    big = np.ascontiguousarray(kg_programme([(0, [(0, 1)])], [], 1))
    mode_rows = np.array([40, 100000], dtype=np.int64)
    offs, rows = (ctypes.c_void_p * 3)(fake, fake, fake), (ctypes.c_void_p * 3)(fake, fake, fake)
    edges = (ctypes.c_int64 * 3)(7, 7, 7)
    Q = 5

    def size(prog=prog, Q=Q, mode_rows=mode_rows, num_modes=2, flags=0):
        return lib.mpqe_kg_workspace_bytes(None if prog is None else prog.ctypes.data, Q,
                                           None if mode_rows is None else mode_rows.ctypes.data, num_modes, flags)

    def call(prog=prog, offs=offs, rows=rows, edges=edges, num_rels=3, mode_rows=mode_rows, num_modes=2, anchors=fake, Q=Q,
             answers=fake, hard=fake, counts=fake, flags=0, ws=fake, wb=1 << 30):
        return lib.mpqe_kg_answers(None if prog is None else prog.ctypes.data, offs, rows, edges, num_rels,
                                   None if mode_rows is None else mode_rows.ctypes.data, num_modes, anchors, Q, answers, hard,
                                   counts, flags, ws, wb, None, None)

    assert size() == 256                                            # LDS form: the workspace is not used
    need = size(flags=_capi.KG_GLOBAL_BITS)
    assert need >= Q * 4 * 2 * 4                                    # four bitmaps of two words per query
    assert size(prog=big) >= Q * 4 * 3125 * 4                       # 100 000 rows: past the LDS form on its own
    assert size(prog=None) == 0 and size(mode_rows=None) == 0 and size(num_modes=0) == 0 and size(num_modes=17) == 0
    assert size(Q=-1) == 0

    assert call(prog=None) == INVALID
    assert call(offs=None) == INVALID and call(rows=None) == INVALID and call(edges=None) == INVALID
    assert call(mode_rows=None) == INVALID
    assert call(num_rels=2) == INVALID                              # the programme names relation 2
    assert call(num_modes=1) == INVALID                             # ... and mode 1
    assert call(anchors=None) == INVALID and call(answers=None) == INVALID
    assert call(Q=-1) == INVALID
    assert call(flags=2) == INVALID
    assert call(edges=(ctypes.c_int64 * 3)(7, -1, 7)) == INVALID
    assert call(offs=(ctypes.c_void_p * 3)(fake, None, fake)) == INVALID
    assert call(flags=_capi.KG_GLOBAL_BITS, ws=None) == INVALID
    assert call(flags=_capi.KG_GLOBAL_BITS, ws=fake + 2) == INVALID
    assert call(flags=_capi.KG_GLOBAL_BITS, wb=need - 257) == WORKSPACE
    assert call(prog=big, wb=1000) == WORKSPACE
    for at, value in ((1, 0), (1, 4), (5, 2), (5, -1), (6, 2), (6, -1), (8, 2), (9, 0), (9, 4), (10, -1), (10, (2 << 4) | 5),
                      (15, (0 << 4) | 1),         # branch 1 ends in mode 1, branch 0 in mode 0
                      (24, (0 << 4) | 1)):        # the last hop ends in mode 1, the target is mode 0
        bad = prog.copy()
        bad[at] = value
        assert call(prog=bad) == INVALID, 'programme[%d] = %d' % (at, value)
        assert size(prog=bad) == 0, 'programme[%d] = %d' % (at, value)
    zero_rows = np.array([40, 0], dtype=np.int64)
    assert call(mode_rows=zero_rows) == INVALID and call(mode_rows=np.array([40, 2 ** 31], dtype=np.int64)) == INVALID
    assert call(Q=0) == OK and call(Q=0, anchors=None, answers=None) == OK          # nothing to do: nothing is launched

    def rows_call(bits=fake, Q=Q, n=40, valid=fake, select=0, offsets=fake, out=fake, cap=10):
        return lib.mpqe_kg_rows(bits, Q, n, valid, select, offsets, out, cap, None, None)
    assert rows_call(bits=None) == INVALID and rows_call(offsets=None) == INVALID and rows_call(out=None) == INVALID
    assert rows_call(Q=-1) == INVALID and rows_call(n=0) == INVALID and rows_call(cap=-1) == INVALID
    assert rows_call(select=3) == INVALID and rows_call(select=-1) == INVALID
    assert rows_call(Q=0) == OK


# ---------------------------------------------------------------------------------------------- the surface on the emulator
@pytest.fixture(scope='module')
def emu_index(tiny):
    from tests.kernel_backend import EmuBackend
    schema, adj, node_maps, graph = tiny
    return KGIndex.from_graph(graph, node_maps, 'cpu', lib=EmuBackend().lib)


def _queries(schema, adj, qt, seed, count=7):
    rng = np.random.RandomState(seed)
    formula = synthetic.sample_formula(schema, qt, rng)
    return formula, synthetic.sample_grounded_queries(schema, adj, formula, count - 2, rng) + \
        synthetic.sample_queries(schema, formula, 2, rng)


@pytest.mark.parametrize('qt', list(_capi.QUERY_TYPE_IDS))
def test_answers_lists_and_csr_forms(tiny, emu_index, qt):
    """index.answers on the emulator: lists / hard_lists / negative_lists and the three CSR forms against the oracle, in
    global entity ids; both homes of the bitmaps give the same words."""
    schema, adj, node_maps, graph = tiny
    formula, queries = _queries(schema, adj, qt, 40 + len(qt))
    ans = emu_index.answers(formula, queries, hard=True)
    want = [kg_oracle.negatives(adj, schema.ids[formula.target_mode], formula, q.anchor_nodes) + (
        kg_oracle.query_sets(adj, formula, q.anchor_nodes)[0],) for q in queries]
    assert [set(l.tolist()) for l in ans.lists()] == [w[2] for w in want]
    assert [set(l.tolist()) for l in ans.hard_lists()] == [w[1] for w in want]
    assert [set(l.tolist()) for l in ans.negative_lists()] == [w[0] for w in want]
    assert ans.counts.tolist() == [[len(w[2]) for w in want], [len(w[1]) for w in want]]
    if 'inter' in qt:
        assert any(w[1] for w in want)
    for (ids, off), col in ((ans.answer_csr(), 2), (ans.hard_csr(), 1), (ans.negative_csr(), 0)):
        for i, w in enumerate(want):
            seg = ids[off[i]:off[i + 1]].tolist()
            assert len(seg) == len(set(seg)) and set(seg) == w[col]
    off, rows = ans.exclusion_csr()
    maps = node_maps.numpy()
    for i, w in enumerate(want):
        assert rows[off[i]:off[i + 1]].tolist() == sorted(int(maps[x]) for x in w[2])
    other = emu_index.answers(formula, np.array([q.anchor_nodes for q in queries]), hard=True, global_bits=True)
    assert torch.equal(other.bits, ans.bits) and torch.equal(other.hard_bits, ans.hard_bits)
    assert torch.equal(other.counts, ans.counts)
    emu_index.check()


def test_an_anchor_of_another_mode_raises_on_check(tiny, emu_index):
    schema, adj, node_maps, graph = tiny
    formula, queries = _queries(schema, adj, '2-inter', 3)
    ids = np.array([q.anchor_nodes for q in queries])
    wrong = [m for m in schema.modes if m != formula.anchor_modes[0]][0]
    ids[2, 0] = schema.ids[wrong][0]
    ans = emu_index.answers(formula, ids)
    lists = ans.lists()
    assert lists[2].size == 0
    for i in (0, 1, 3):
        assert set(lists[i].tolist()) == kg_oracle.query_sets(adj, formula, queries[i].anchor_nodes)[0]
    with pytest.raises(IndexError):
        emu_index.check()
    emu_index.check()                   # (the word was cleared)


class _StubModel(object):
    def __init__(self, index_rows):
        self.seen, self.index_rows = [], index_rows

    def rank_targets(self, formula, queries, targets, exclude=None):
        from mpqe_amd.kg import KGAnswers
        if isinstance(exclude, KGAnswers):
            off, rows = exclude.exclusion_csr()
            lists = [rows[off[i]:off[i + 1]].tolist() for i in range(len(queries))]
        else:
            lists = [sorted(set(self.index_rows(formula.target_mode, np.asarray(e, dtype=np.int64)).tolist())) for e in exclude]
        self.seen.append((formula, [q.target_node for q in queries], lists))
        return torch.arange(1, len(queries) + 1)


def test_eval_rank_queries_hands_the_models_the_same_exclusions(tiny, emu_index):
    """eval_rank_queries(known_answers=index) against known_answers = the dict of synthetic._answers sets: the model is
    handed the same rows to exclude for every batch (the tiny KG's tables have no holes), and the metrics agree."""
    from mpqe_amd.evaluation import eval_rank_queries
    schema, adj, node_maps, graph = tiny
    test_queries = {}
    for k, qt in enumerate(_capi.QUERY_TYPE_IDS):
        formula, queries = _queries(schema, adj, qt, 70 + k, count=5)
        test_queries[formula] = queries
    known = {q: synthetic._answers(adj, f, list(q.anchor_nodes))[0] for f, qs in test_queries.items() for q in qs}
    by_dict, by_index = _StubModel(emu_index._rows_of), _StubModel(emu_index._rows_of)
    a = eval_rank_queries(test_queries, by_dict, batch_size=3, known_answers=known)
    b = eval_rank_queries(test_queries, by_index, batch_size=3, known_answers=emu_index)
    assert a == b and a['num_queries'] == 5 * len(test_queries)
    assert by_dict.seen == by_index.seen and len(by_dict.seen) == 2 * len(test_queries) >= 12
    assert any(l for _, _, lists in by_dict.seen for l in lists)
    emu_index.check()


def test_negative_sampler_from_csr_holds_the_lists(tiny, emu_index):
    from mpqe_amd.sampling import NegativeSampler
    schema, adj, node_maps, graph = tiny
    formula, queries = _queries(schema, adj, '3-inter', 9)
    ans = emu_index.answers(formula, queries, hard=True)
    s = NegativeSampler.from_csr(ans.negative_csr(), ans.hard_csr(), 'cpu')
    assert s.n == len(queries) and s.shared is None
    assert s.neg[1].tolist() == ans.negative_csr()[1].tolist() and s.hard[0].tolist() == ans.hard_csr()[0].tolist()
    with pytest.raises(ValueError):
        NegativeSampler.from_csr(ans.negative_csr(), (ans.hard_csr()[0], ans.hard_csr()[1][:-1]), 'cpu')
