"""The host side of answering a query: eval_rank_queries' metric arithmetic and batching on a stub model, and the
argument checks of ops.rank_entities that come before any device is touched. No GPU needed."""
import numpy as np
import pytest
import torch

from mpqe_amd import evaluation, ops


class _Q(object):
    def __init__(self, target, rank):
        self.target_node = target
        self.rank = rank


class _Stub(object):
    """rank_targets hands back the rank written on each query, minus one per known answer handed in (the target
    excepted), and records the calls."""

    def __init__(self):
        self.calls = []

    def rank_targets(self, formula, queries, target_nodes=None, exclude=None, **kw):
        assert target_nodes == [q.target_node for q in queries]
        self.calls.append((formula, len(queries), None if exclude is None else [list(e) for e in exclude]))
        ranks = [q.rank for q in queries]
        if exclude is not None:
            ranks = [max(1, r - len([x for x in e if x != q.target_node])) for r, e, q in zip(ranks, exclude, queries)]
        return torch.tensor(ranks, dtype=torch.int64)


def test_metrics_and_batching():
    rng = np.random.RandomState(0)
    tq = {'f1': [_Q(i, int(r)) for i, r in enumerate(rng.randint(1, 30, size=300))],
          'f2': [_Q(i, int(r)) for i, r in enumerate(rng.randint(1, 5, size=7))]}
    stub = _Stub()
    out = evaluation.eval_rank_queries(tq, stub, batch_size=128, ks=(1, 3, 10))
    assert [(f, n) for f, n, _ in stub.calls] == [('f1', 128), ('f1', 128), ('f1', 44), ('f2', 7)]
    assert all(e is None for _, _, e in stub.calls)
    for name, qs in list(tq.items()) + [('all', tq['f1'] + tq['f2'])]:
        r = np.array([q.rank for q in qs], dtype=np.float64)
        got = out if name == 'all' else out['per_formula'][name]
        assert got['num_queries'] == len(qs)
        np.testing.assert_allclose(got['mrr'], np.mean(1.0 / r), rtol=1e-12)
        for k in (1, 3, 10):
            np.testing.assert_allclose(got['hits@%d' % k], np.mean(r <= k), rtol=1e-12)
    assert set(out) == {'mrr', 'hits@1', 'hits@3', 'hits@10', 'num_queries', 'per_formula'}


def test_known_answers_are_passed_per_query():
    qs = [_Q(10, 4), _Q(11, 9), _Q(12, 1)]
    known = {qs[0]: {10, 50, 51}, qs[1]: {11}, qs[2]: {12, 60}}
    stub = _Stub()
    out = evaluation.eval_rank_queries({'f': qs}, stub, batch_size=2, ks=(1,), known_answers=known)
    assert [n for _, n, _ in stub.calls] == [2, 1]
    assert sorted(stub.calls[0][2][0]) == [10, 50, 51] and stub.calls[0][2][1] == [11] and sorted(stub.calls[1][2][0]) == [12, 60]
    np.testing.assert_allclose(out['mrr'], np.mean([1 / 2.0, 1 / 9.0, 1.0]))
    assert out['hits@1'] == pytest.approx(1 / 3.0)


def test_empty_query_set():
    out = evaluation.eval_rank_queries({}, _Stub())
    assert out['num_queries'] == 0 and np.isnan(out['mrr']) and out['per_formula'] == {}


def test_rank_entities_checks_arguments_before_the_device():
    q, t = torch.zeros(3, 8), torch.zeros(5, 8)
    rows = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(ValueError):
        ops.rank_entities(q, t, rows, k=-1)
    with pytest.raises(ValueError):
        ops.rank_entities(q, t, rows, k=ops.RANK_MAX_K + 1)
    with pytest.raises(ValueError):
        ops.rank_entities(q, torch.zeros(5, 9), rows, k=2)              # dims differ
    with pytest.raises(ValueError):
        ops.rank_entities(q, torch.zeros(0, 8), rows, k=2)              # no rows
    with pytest.raises(ValueError):
        ops.rank_entities(q, t, torch.zeros(4, dtype=torch.int64), k=2)  # one target per query
    with pytest.raises(ValueError):
        ops.rank_entities(q, t, None, k=0)                              # nothing asked for
    with pytest.raises(ValueError):
        ops.rank_entities(q, t, rows, exclude=[[1], [2]], k=2)          # one list per query
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.rank_entities(q, t, rows, k=2)                              # host tensors: refused, not computed on the CPU


def test_exclusion_csr_sorts_and_removes_repeats():
    off, rows = ops.exclusion_csr([[5, 1, 5, 3], [], [2]], 3)
    assert off.tolist() == [0, 3, 3, 4] and rows.tolist() == [1, 3, 5, 2]
    assert off.dtype == np.int64 and rows.dtype == np.int64
