"""mpqe_rgcn_fwd_mixed_save / mpqe_rgcn_bwd_mixed / mpqe_rgcn_mixed_index_build (csrc/rgcn_mixed_train.h) through the C ABI,
on the host emulator and on the GPU (the `be` fixture of tests/test_gqe_kernels.py): training the R-GCN model on queries of
DIFFERENT formulas of one query type. Problems are tests/test_rgcn_mixed_kernels.Problem's; every operand, block and
workspace sits between fences (tests/fenced.py).

The window: runs (formula, length) = (0,1) (1,63) (2,64) (3,65) (4,1) (5,1) (0,3), Q = 198 -- stretches end one short of,
at and one past a 64-query block, a chunk of 64 contributions is met at 63 / 64 / 65, formula 0 returns (a parameter gets
terms from two separate runs); negative counts cycle 0, 1, 2, 65; the same entity is an anchor in two formulas, a target in
two formulas, and an anchor and a target of one table (share_ids).

Oracle: tests/rgcn_mixed_oracle.run in float64 (tolerances FWD / BWD of tests/gqe_oracle.py). The toleranced problems are
searched as gqe_common.settled_problem searches: the float64 oracle alone finds no ReLU pre-activation and no max-readout
gap within gc.TIE_TOL, its float32 twin stays within half of FWD / BWD, at most 50 seeds, 0 queries dropped. In the exact
problems every value is an exactly representable number (one-hot +-2^k table rows, integer mode embeddings, weights and
grad_q), asserted by the float32 twin equalling the float64 oracle, so the order of a sum cannot matter and every gradient
is compared with array_equal."""
import ctypes

import numpy as np
import pytest

from mpqe_amd import _capi
from tests import rgcn_mixed_oracle as ro
from tests import test_rgcn_mixed_kernels as mk
from tests.fenced import FILLS, assert_fence_intact, fenced, fenced_bytes
from tests.gqe_oracle import BWD, FWD
from tests.test_gqe_kernels import INVALID, OK, TYPES, UNSUPPORTED, WORKSPACE, be  # noqa: F401  (`be`: the backend fixture)

RUNS = ((0, 1), (1, 63), (2, 64), (3, 65), (4, 1), (5, 1), (0, 3))
NEGS = (0, 1, 2, 65)
F = 6
C = _capi.RGCN_MIX_GRAD_CHUNK
MODES, RELS = mk.MODES, mk.RELS
FLAG_BAD_NODE_ID, FLAG_BAD_RELATION, FLAG_BAD_INDEX = 1, 4, 8


def share_ids(prob):
    """the same entity as an anchor in two formulas, as a target in two formulas, and as an anchor and a target of one
    table -> the set of what was arranged"""
    done = {}
    first = {}
    for q in range(prob.Q):
        first.setdefault(int(prob.formula_of[q]), q)
    reps = sorted(first.values())
    for q1 in reps:
        for q2 in reps:
            r1, r2 = prob.recs[prob.formula_of[q1]], prob.recs[prob.formula_of[q2]]
            if q1 >= q2:
                continue
            if 'anchor' not in done and r1[3] == r2[3]:
                prob.anchors[q2, 0] = prob.anchors[q1, 0]
                done['anchor'] = (q1, q2)
            elif 'target' not in done and r1[9] == r2[9] and q1 not in done.get('anchor', ()) and q2 not in done.get('anchor', ()):
                prob.targets[q2] = prob.targets[q1]
                done['target'] = (q1, q2)
    used = {q for pair in done.values() for q in pair}
    for q1 in range(prob.Q):
        for q2 in range(prob.Q):
            if 'both' in done or q1 == q2 or q1 in used or q2 in used:
                continue
            if prob.recs[prob.formula_of[q1]][3] == prob.recs[prob.formula_of[q2]][9]:
                prob.targets[q2] = prob.anchors[q1, 0]
                done['both'] = (q1, q2)
    prob.pair_ids[:prob.Q] = prob.targets
    return set(done)


def within_half(a, b, tol):
    return bool((np.abs(a - b) <= 0.5 * (tol['atol'] + tol['rtol'] * np.abs(b))).all())


_SETTLED = {}


def make(qt, D, seed, **kw):
    prob = mk.Problem(qt, D, F, RUNS, seed, neg_counts=NEGS, **kw)
    assert share_ids(prob) == {'anchor', 'target', 'both'}
    return prob


def settled(qt, D, readout='mp', layers=3, bias=True, passes=None):
    """(problem, float64 oracle result): the first of at most 50 seeds the search of the module docstring accepts.
    Computed once, shared by both backends."""
    key = (qt, D, readout, layers, bias, passes)
    if key in _SETTLED:
        return _SETTLED[key]
    first = 1000 * TYPES.index(qt) + D
    for s in range(first, first + 50):
        prob = make(qt, D, s, readout=readout, layers=layers, bias=bias, passes=passes)
        prob.grad_scores = np.random.RandomState(s + 7).normal(0, 1.0, prob.n).astype(np.float32)
        o = ro.run(prob, np.float64, grad_scores=prob.grad_scores)
        if o.ties:
            continue
        o32 = ro.run(prob, np.float32, grad_scores=prob.grad_scores)
        if within_half(o32.scores, o.scores, FWD) and all(within_half(o32.grads[k], o.grads[k], BWD) for k in o.grads):
            _SETTLED[key] = (prob, o)
            return _SETTLED[key]
    raise AssertionError('no seed without near-ties')


def make_exact(prob, seed):
    """one-hot +-2^k table rows, small integer mode embeddings, weights and grad_q (D 16) -> (problem, float64 oracle)"""
    rng = np.random.RandomState(seed + 11)
    for t in prob.tables:
        t[...] = 0
        rows = np.arange(t.shape[0])
        t[rows, rng.randint(0, 16, size=t.shape[0])] = rng.choice([-1.0, 1.0], size=t.shape[0]) * 2.0 ** rng.randint(-2, 3, size=t.shape[0])
    prob.mode_emb[...] = rng.randint(-1, 2, size=prob.mode_emb.shape)
    for b, r, bi in prob.layers:
        b[...] = rng.choice([-1.0, 0.0, 1.0], p=[0.15, 0.7, 0.15], size=b.shape)
        r[...] = rng.choice([-1.0, 0.0, 1.0], p=[0.15, 0.7, 0.15], size=r.shape)
        bi[...] = rng.randint(-1, 2, size=bi.shape)
    prob.grad_q = rng.randint(-2, 3, size=(prob.Q, 16)).astype(np.float32)
    o = ro.run(prob, np.float64, grad_q=prob.grad_q)
    o32 = ro.run(prob, np.float32, grad_q=prob.grad_q)
    # every intermediate is an exactly representable number: the float32 twin IS the float64 oracle
    np.testing.assert_array_equal(o32.q.astype(np.float64), o.q)
    for k in o.grads:
        np.testing.assert_array_equal(o32.grads[k].astype(np.float64), o.grads[k], err_msg=k)
    assert any(g.any() for g in o.grads.values())
    return prob, o


def exact_problem(qt, readout='mp', layers=3, passes=None, seed=5):
    key = ('exact', qt, readout, layers, passes, seed)
    if key not in _SETTLED:
        _SETTLED[key] = make_exact(make(qt, 16, seed, readout=readout, layers=layers, passes=passes), seed)
    return _SETTLED[key]


class Train(mk.Device):
    """A problem's shared operands on a backend plus the index block, the training workspace and the three calls."""

    def __init__(self, be, prob):
        super(Train, self).__init__(be, prob)
        self.L = len(prob.layers)
        self.nm = int(self.node_map.shape[0])
        self.lop = (ctypes.c_int * prob.passes)(*prob.layer_of_pass)

    def build_index(self, fill='nan', short=0):
        be, prob = self.be, self.prob
        self.index_bytes = be.lib.mpqe_rgcn_mixed_index_bytes(prob.recs.shape[0])
        assert self.index_bytes > 0 and self.index_bytes % 256 == 0
        self.index = fenced_bytes(be, self.index_bytes - short, fill)
        recs = np.ascontiguousarray(prob.recs, dtype=np.int32)
        return be.lib.mpqe_rgcn_mixed_index_build(prob.qid, recs.ctypes.data, recs.shape[0], be.ptr(self.index),
                                                  self.index_bytes - short, be.stream)

    def ready(self):
        assert self.build() == OK and self.build_index() == OK
        return self

    def place(self, fill='nan', short=0, misalign=0, formula_of=None, anchors=None, pair_ids=None, Q=None, n=None,
              neg_off=None):
        be, prob = self.be, self.prob
        self.Q = prob.Q if Q is None else Q
        self.n = prob.n if n is None else n
        self.keep = [mk.place(be, prob.formula_of if formula_of is None else formula_of),
                     mk.place(be, prob.anchors if anchors is None else anchors),
                     mk.place(be, prob.pair_ids if pair_ids is None else pair_ids),
                     mk.place(be, prob.neg_off if neg_off is None else neg_off)]
        self.scores = mk.place(be, np.full(self.n, np.float32(7.5)))
        self.q_out = mk.place(be, np.full((self.Q, prob.D), np.float32(7.5)))
        self.wb = be.lib.mpqe_rgcn_mixed_train_workspace_bytes(prob.qid, self.Q, self.n, prob.D, self.passes, RELS, MODES,
                                                               MODES, self.L) if self.Q else 256
        assert self.wb > 0 and self.wb % 256 == 0
        self.ws = fenced_bytes(be, self.wb - short, fill, misalign=misalign)
        self.short = short
        z = lambda a: None if a is None else fenced(be, np.zeros(tuple(a.shape), np.float32))
        self.g = {'mode_emb': z(prob.mode_emb)}
        for m, t in enumerate(prob.tables):
            self.g['table%d' % m] = z(t)
        for l, (b, r, bi) in enumerate(prob.layers):
            self.g['basis%d' % l], self.g['root%d' % l] = z(b), z(r)
            if bi is not None:
                self.g['bias%d' % l] = z(bi)
        return self

    def _head(self, **over):
        be, prob = self.be, self.prob
        a = dict(qid=prob.qid, F=prob.F, desc=be.ptr(self.desc), desc_bytes=self.desc_bytes, node_map=be.ptr(self.node_map),
                 mode_emb=be.ptr(self.mode_emb), basis=self.basis, root=self.root, bias=self.bias, R=RELS, passes=self.passes,
                 readout=mk.READOUTS[prob.readout], D=prob.D, fo=be.ptr(self.keep[0]), an=be.ptr(self.keep[1]), Q=self.Q,
                 ids=be.ptr(self.keep[2]), neg_off=be.ptr(self.keep[3]), n=self.n, T=MODES, M=MODES, L=self.L,
                 ws=be.ptr(self.ws), wb=self.wb - self.short, index=be.ptr(self.index) if hasattr(self, 'index') else None,
                 index_bytes=getattr(self, 'index_bytes', 0), lop=self.lop)
        a.update(over)
        return a

    def forward(self, q_out=False, **over):
        be = self.be
        a = self._head(**over)
        return be.lib.mpqe_rgcn_fwd_mixed_save(
            a['qid'], a['F'], a['desc'], a['desc_bytes'], a['node_map'], self.nm, a['mode_emb'], a['basis'], a['root'],
            a['bias'], a['R'], a['passes'], a['readout'], a['D'], a['fo'], a['an'], a['Q'], a['ids'], a['neg_off'], a['n'], 1e-8,
            a['T'], a['M'], a['L'], a['ws'], a['wb'], be.ptr(self.scores), be.ptr(self.q_out) if q_out else None,
            be.ptr(self.err), be.stream)

    def backward(self, grad_scores=None, grad_q=None, null=(), both=False, neither=False, **over):
        be, prob = self.be, self.prob
        a = self._head(**over)
        self.gs = None if grad_scores is None else mk.place(be, grad_scores)
        self.gq = None if grad_q is None else mk.place(be, grad_q)
        ptr = lambda k: None if (k in null or self.g.get(k) is None) else be.ptr(self.g[k])
        gt = (ctypes.c_void_p * MODES)(*[ptr('table%d' % m) for m in range(MODES)])
        per = lambda what: (ctypes.c_void_p * self.L)(*[ptr('%s%d' % (what, l)) for l in range(self.L)])
        gs, gq = be.ptr(self.gs), be.ptr(self.gq)
        if both:
            gs = gq = be.ptr(self.scores)
        if neither:
            gs = gq = None
        return be.lib.mpqe_rgcn_bwd_mixed(
            a['qid'], a['F'], a['desc'], a['desc_bytes'], a['index'], a['index_bytes'], a['node_map'], self.nm, a['mode_emb'],
            a['basis'], a['root'], a['bias'], a['R'], a['passes'], a['readout'], a['D'], a['fo'], a['an'], a['Q'], a['ids'],
            a['neg_off'], a['n'], 1e-8, a['T'], a['M'], a['L'], a['lop'], gs, gq, gt, ptr('mode_emb'), per('basis'),
            per('root'), per('bias'), a['ws'], a['wb'], be.ptr(self.err), be.stream)

    def grads(self):
        """{oracle key: array}; every fence checked on the way"""
        be = self.be
        out = {}
        for k, g in self.g.items():
            if g is None:
                continue
            assert_fence_intact(be, g, 'grad ' + k)
            out[k] = be.get(g).copy()
        for what in ('ws', 'desc', 'index'):
            assert_fence_intact(be, getattr(self, what), what)
        for t in [self.scores, self.q_out] + self.keep + self.tables + [self.mode_emb, self.node_map]:
            if t.size if be.name == 'emu' else t.numel():
                assert_fence_intact(be, t, 'operand')
        for b, r, bi in self.layers:
            for t in (b, r) + (() if bi is None else (bi,)):
                assert_fence_intact(be, t, 'layer')
        return out


def assert_close(o, scores, grads):
    np.testing.assert_allclose(scores, o.scores, **FWD)
    assert sorted(grads) == sorted(o.grads)
    for k, g in grads.items():
        print('%s: max abs error %.3g (max |ref| %.3g)' % (k, np.abs(g - o.grads[k]).max(), np.abs(o.grads[k]).max()))
        np.testing.assert_allclose(g, o.grads[k], err_msg=k, **BWD)
    assert any(g.any() for k, g in grads.items() if k.startswith('table'))
    assert grads['mode_emb'].any() and any(g.any() for k, g in grads.items() if k.startswith('basis'))


def check_toleranced(be, prob, o):
    assert prob.Q == 198 and sorted(set(prob.neg_lengths)) == sorted(NEGS) and len(prob.runs()) == 7
    dev = Train(be, prob).ready().place()
    assert dev.forward() == OK
    assert dev.backward(grad_scores=prob.grad_scores) == OK
    assert int(be.get(dev.err)[0]) == 0
    scores = be.get(dev.scores).copy()
    assert_close(o, scores, dev.grads())
    # the save call's scores are mpqe_rgcn_fwd_mixed's, bit for bit
    dev.workspace()
    st, plain = dev.mixed()
    assert st == OK
    np.testing.assert_array_equal(mk.bits(scores), mk.bits(be.get(plain)))
    return dev


# ------------------------------------------------------------------------------------------------ toleranced cases
def test_symbols_and_sizes(be):
    for name in ('mpqe_rgcn_mixed_index_bytes', 'mpqe_rgcn_mixed_index_build', 'mpqe_rgcn_mixed_train_workspace_bytes',
                 'mpqe_rgcn_fwd_mixed_save', 'mpqe_rgcn_bwd_mixed'):
        assert name in _capi.PROTOTYPES and hasattr(be.lib, name)
    assert be.lib.mpqe_abi_version() == 7
    assert be.lib.mpqe_rgcn_mixed_index_bytes(0) == 0 and be.lib.mpqe_rgcn_mixed_index_bytes(1) == 256
    size = be.lib.mpqe_rgcn_mixed_train_workspace_bytes
    assert size(2, 5, 10, 48, 3, 5, 3, 3, 3) > 0
    for bad in ((7, 5, 10, 48, 3, 5, 3, 3, 3), (2, 0, 0, 48, 3, 5, 3, 3, 3), (2, 5, 4, 48, 3, 5, 3, 3, 3), (2, 5, 10, 40, 3, 5, 3, 3, 3),
                (2, 5, 10, 272, 3, 5, 3, 3, 3), (2, 5, 10, 48, 5, 5, 3, 3, 3), (2, 5, 10, 48, 3, 0, 3, 3, 3),
                (2, 5, 10, 48, 3, 5, 0, 3, 3), (2, 5, 10, 48, 3, 5, 3, 0, 3), (2, 5, 10, 48, 3, 5, 3, 3, 0)):
        assert size(*bad) == 0, bad


@pytest.mark.parametrize('qt', TYPES)
def test_every_type_against_float64(be, qt):
    prob, o = settled(qt, 16)
    check_toleranced(be, prob, o)


@pytest.mark.parametrize('D', [48, 128])
@pytest.mark.parametrize('qt', ['3-inter_chain', '3-chain_inter'])
def test_wider_rows_against_float64(be, qt, D):
    prob, o = settled(qt, D)
    check_toleranced(be, prob, o)


@pytest.mark.parametrize('readout', ['sum', 'max'])
@pytest.mark.parametrize('qt', ['2-chain', '3-inter'])
def test_sum_and_max_readouts(be, qt, readout):
    prob, o = settled(qt, 16, readout=readout)
    check_toleranced(be, prob, o)


@pytest.mark.parametrize('passes,layers', [(1, 1), (4, 1), (1, 3), (4, 3), (None, 1)])
def test_passes_and_shared_layers(be, passes, layers):
    """one shared layer (every pass adds to the same buffers) and three distinct ones; passes 1 and 4"""
    prob, o = settled('3-inter_chain', 16, layers=layers, passes=passes)
    assert prob.layer_of_pass == ([0] * prob.passes if layers == 1 else [0, 1, 2, 2][:prob.passes - 1] + [2])
    check_toleranced(be, prob, o)


def test_bias_absent(be):
    prob, o = settled('2-inter', 16, bias=False)
    assert not any(k.startswith('bias') for k in o.grads)
    check_toleranced(be, prob, o)


# ------------------------------------------------------------------------------------------------ exact cases
def run_exact(be, prob, fill='nan', null=(), grad_q=None, **window):
    """the save call without pairs (n = 0) + the backward through grad_q -> (device, gradients)"""
    dev = Train(be, prob).ready().place(fill=fill, n=0, **window)
    assert dev.forward(q_out=True) == OK
    assert dev.backward(grad_q=prob.grad_q if grad_q is None else grad_q, null=null) == OK
    return dev, dev.grads()


EXACT = [('1-chain', 'mp', 3), ('2-chain', 'sum', 1), ('3-chain', 'mp', 3), ('2-inter', 'max', 3), ('3-inter', 'mp', 1),
         ('3-inter_chain', 'sum', 3), ('3-chain_inter', 'max', 1)]


@pytest.mark.parametrize('qt,readout,layers', EXACT)
def test_exact_gradients(be, qt, readout, layers):
    prob, o = exact_problem(qt, readout, layers)
    dev, grads = run_exact(be, prob)
    assert int(be.get(dev.err)[0]) == 0
    np.testing.assert_array_equal(be.get(dev.q_out).astype(np.float64), o.q)
    assert sorted(grads) == sorted(o.grads)
    for k in grads:
        np.testing.assert_array_equal(grads[k].astype(np.float64), o.grads[k], err_msg=k)


@pytest.mark.parametrize('count', [C - 1, C, C + 1, 2 * C + 1])
def test_one_relation_at_the_chunk_edges(be, count):
    """a 1-chain under the target-message readout is one pass of one layer with one edge into the target slot: `count`
    queries of one relation (two formulas, in two runs, so that the window is not one run) give that relation's basis
    matrix, the root matrix and the bias exactly `count` contributions each -- one 16-row strip, one wave at D 16"""
    key = ('edge', count)
    if key not in _SETTLED:
        prob = mk.Problem('1-chain', 16, 2, ((0, count - 3), (1, 3)), 5, readout='mp', layers=1, neg_counts=(0,))
        prob.recs[:, 0] = prob.recs[0, 0]
        _SETTLED[key] = make_exact(prob, 5)
    prob, o = _SETTLED[key]
    assert prob.Q == count and prob.passes == 1 and len(prob.layers) == 1
    assert o.grads['basis0'].reshape(RELS, -1).any(axis=1).sum() == 1 and o.grads['root0'].any() and o.grads['bias0'].any()
    dev, grads = run_exact(be, prob)
    assert int(be.get(dev.err)[0]) == 0
    assert sorted(grads) == sorted(o.grads)
    for k in grads:
        np.testing.assert_array_equal(grads[k].astype(np.float64), o.grads[k], err_msg=k)


@pytest.mark.parametrize('bad', [-1, F, 2 ** 40])
def test_bad_formula_index_is_the_window_without_the_query(be, bad):
    prob, o = exact_problem('3-inter_chain', 'sum', 3)
    victim = 70                                     # (inside the run of 64: it is cut in two)
    fo = prob.formula_of.copy()
    fo[victim] = bad
    dev, grads = run_exact(be, prob, formula_of=fo)
    assert int(be.get(dev.err)[0]) == FLAG_BAD_INDEX
    keep = np.arange(prob.Q) != victim
    gq = prob.grad_q.copy()
    gq[victim] = 0                                  # (the oracle of the window without the query)
    want = ro.run(prob, np.float64, grad_q=gq, formula_of=fo)
    for k in grads:
        np.testing.assert_array_equal(grads[k].astype(np.float64), want.grads[k], err_msg=k)
    # ... and the library's own window with that query removed
    sub = Train(be, prob).ready().place(n=0, formula_of=prob.formula_of[keep], anchors=prob.anchors[keep], Q=prob.Q - 1)
    assert sub.forward() == OK and sub.backward(grad_q=prob.grad_q[keep]) == OK
    removed = sub.grads()
    for k in grads:
        np.testing.assert_array_equal(grads[k], removed[k], err_msg=k)


def test_bad_relation(be):
    """a relation past the call's count: the flag, its formulas give no gradient, the others are unaffected (exact)"""
    prob, o = exact_problem('2-chain', 'mp', 3)
    low = int(prob.recs[:, 0:prob.E].max())
    dev = Train(be, prob).ready().place(n=0)
    assert dev.forward(R=low) == OK and dev.backward(grad_q=prob.grad_q, R=low) == OK
    assert int(be.get(dev.err)[0]) == FLAG_BAD_RELATION
    want = ro.run(prob, np.float64, grad_q=prob.grad_q, R=low)
    # (the buffers keep their shape: the relations past `low` get nothing)
    got = dev.grads()
    for k in got:
        np.testing.assert_array_equal(got[k].astype(np.float64), want.grads[k], err_msg=k)
    assert any(g.any() for g in got.values())


def test_bad_anchor_id_exact(be):
    """a bad anchor id on the exact problem, through grad_q: the flag, the anchor's row is zeros (the oracle's lookup), no
    table gradient from it, every other bit as the oracle's -- and where the gradients of the clean window differ is
    confined to what that query reaches"""
    prob, o = exact_problem('3-inter_chain', 'sum', 3)
    no_mode = prob.node_map.shape[0] - 1          # (in the map, of no mode: -1)
    anchors = prob.anchors.copy()
    anchors[70, 0] = no_mode
    anchors[3, prob.A - 1] = 10 ** 12
    dev, grads = run_exact(be, prob, anchors=anchors)
    assert int(be.get(dev.err)[0]) == FLAG_BAD_NODE_ID
    want = ro.run(prob, np.float64, grad_q=prob.grad_q, anchors=anchors)
    want32 = ro.run(prob, np.float32, grad_q=prob.grad_q, anchors=anchors)
    np.testing.assert_array_equal(be.get(dev.q_out).astype(np.float64), want.q)
    for k in grads:
        np.testing.assert_array_equal(want32.grads[k].astype(np.float64), want.grads[k], err_msg=k)      # (still exact)
        np.testing.assert_array_equal(grads[k].astype(np.float64), want.grads[k], err_msg=k)
    # the other queries' embeddings are the clean window's bits
    others = np.ones(prob.Q, dtype=bool)
    others[[70, 3]] = False
    np.testing.assert_array_equal(mk.bits(be.get(dev.q_out)[others]), mk.bits(o.q[others].astype(np.float32)))
    assert any((grads[k].astype(np.float64) != o.grads[k]).any() for k in grads)


def test_bad_target_ids_toleranced(be):
    """bad target / negative ids need the score phase (the cosine is no exact arithmetic): the flag, score 0, no table
    gradient from them. The changed inputs are searched again for near ties before they are relied on."""
    prob, o = settled('2-chain', 16)
    no_mode = prob.node_map.shape[0] - 1
    pair_ids = prob.pair_ids.copy()
    pair_ids[5] = no_mode
    pair_ids[prob.Q + 9] = -4
    want = ro.run(prob, np.float64, grad_scores=prob.grad_scores, pair_ids=pair_ids)
    want32 = ro.run(prob, np.float32, grad_scores=prob.grad_scores, pair_ids=pair_ids)
    assert want.ties == 0 and within_half(want32.scores, want.scores, FWD)
    assert all(within_half(want32.grads[k], want.grads[k], BWD) for k in want.grads)
    dev = Train(be, prob).ready().place(pair_ids=pair_ids)
    assert dev.forward() == OK and dev.backward(grad_scores=prob.grad_scores) == OK
    assert int(be.get(dev.err)[0]) == FLAG_BAD_NODE_ID
    got = be.get(dev.scores)
    assert got[5] == 0 and got[prob.Q + 9] == 0
    np.testing.assert_allclose(got, want.scores, **FWD)
    for k, g in dev.grads().items():
        np.testing.assert_allclose(g, want.grads[k], err_msg=k, **BWD)
    # the other pairs' scores are the clean window's bits
    clean = Train(be, prob).ready().place()
    assert clean.forward() == OK
    others = np.ones(prob.n, dtype=bool)
    others[[5, prob.Q + 9]] = False
    np.testing.assert_array_equal(mk.bits(got[others]), mk.bits(be.get(clean.scores)[others]))


# ------------------------------------------------------------------------------------------------ determinism, skipping
def test_two_calls_on_different_garbage_give_equal_bits(be):
    prob, o = settled('3-chain_inter', 48)
    runs = []
    for fill in ('ones', 'noise'):
        dev = Train(be, prob).ready().place(fill=fill)
        assert dev.forward() == OK and dev.backward(grad_scores=prob.grad_scores) == OK
        runs.append((be.get(dev.scores).tobytes(), {k: g.tobytes() for k, g in dev.grads().items()}))
    assert runs[0] == runs[1]


def test_null_pointers_skip_and_gradients_are_added(be):
    prob, o = exact_problem('3-inter_chain', 'sum', 3)
    dev, full = run_exact(be, prob)
    for null in (('table1',), ('mode_emb',), ('basis0', 'bias2'), ('root1', 'root2', 'basis2')):
        dev, grads = run_exact(be, prob, null=null)
        for k in grads:
            if k in null:
                assert not grads[k].any(), k
            else:
                np.testing.assert_array_equal(grads[k], full[k], err_msg=k)
    # a second backward on the same buffers adds
    assert dev.backward(grad_q=prob.grad_q) == OK
    twice = dev.grads()
    for k in twice:
        np.testing.assert_array_equal(twice[k], full[k] if k in null else full[k] + full[k], err_msg=k)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_come_before_anything_is_written(be):
    prob, o = settled('3-inter', 16)
    dev = Train(be, prob).ready().place(fill='noise')
    image = be.get(dev.ws).copy()
    gs = prob.grad_scores
    cases = [(UNSUPPORTED, dict(D=24)), (UNSUPPORTED, dict(D=272)), (UNSUPPORTED, dict(passes=0)), (UNSUPPORTED, dict(passes=5)),
             (UNSUPPORTED, dict(readout=3)), (INVALID, dict(ws=be.ptr(dev.ws) + 16)), (INVALID, dict(ws=None)),
             (INVALID, dict(qid=7)), (INVALID, dict(F=0)), (INVALID, dict(desc=None)), (INVALID, dict(fo=None)),
             (INVALID, dict(desc=be.ptr(dev.desc) + 16)),
             (INVALID, dict(T=0)), (INVALID, dict(M=0)), (INVALID, dict(L=0)), (UNSUPPORTED, dict(L=5)),
             (WORKSPACE, dict(wb=dev.wb - 1)), (WORKSPACE, dict(desc_bytes=dev.desc_bytes - 1))]
    bwd_only = [(INVALID, dict(index=None)), (INVALID, dict(index=be.ptr(dev.index) + 16)),
                (WORKSPACE, dict(index_bytes=dev.index_bytes - 1)),
                (INVALID, dict(lop=(ctypes.c_int * prob.passes)(*([0] * (prob.passes - 1) + [3])))),
                (INVALID, dict(lop=(ctypes.c_int * prob.passes)(*([-1] + [0] * (prob.passes - 1))))), (INVALID, dict(lop=None))]
    for status, over in cases:
        assert dev.forward(**over) == status, over
        assert dev.backward(grad_scores=gs, **over) == status, over
    for status, over in bwd_only:
        assert dev.backward(grad_scores=gs, **over) == status, over
    assert dev.backward(grad_scores=gs, both=True) == INVALID and dev.backward(neither=True) == INVALID
    assert (be.get(dev.scores) == np.float32(7.5)).all()
    np.testing.assert_array_equal(be.get(dev.ws), image)
    assert not any(g.any() for g in dev.grads().values())
    assert int(be.get(dev.err)[0]) == 0
    # a workspace a byte short, an index block a byte short: refused with the fences intact
    short = Train(be, prob).ready().place(fill='noise', short=1)
    before = be.get(short.ws).copy()
    assert short.forward() == WORKSPACE and short.backward(grad_scores=gs) == WORKSPACE
    np.testing.assert_array_equal(be.get(short.ws), before)
    assert_fence_intact(be, short.ws, 'workspace')
    assert short.build_index(fill='noise', short=1) == WORKSPACE
    np.testing.assert_array_equal(be.get(short.index), np.resize(FILLS['noise'], short.index_bytes - 1))
    assert_fence_intact(be, short.index, 'index')
    # a workspace that is not 256-byte aligned
    off = Train(be, prob).ready().place(fill='noise', misalign=64)
    assert off.forward() == INVALID and off.backward(grad_scores=gs) == INVALID
    assert_fence_intact(be, off.ws, 'workspace')


@pytest.mark.parametrize('fill', sorted(FILLS))
def test_exact_size_blocks_whatever_they_held(be, fill):
    prob, o = exact_problem('3-inter', 'mp', 1)
    dev, grads = run_exact(be, prob, fill=fill)
    for k in grads:
        np.testing.assert_array_equal(grads[k].astype(np.float64), o.grads[k], err_msg=k)


def test_no_queries(be):
    prob = mk.Problem('2-inter', 16, 2, (), 43)
    dev = Train(be, prob).ready().place()
    assert dev.forward(ws=None) == OK
    assert dev.backward(grad_q=np.zeros((1, 16), np.float32), ws=None) == OK
    assert int(be.get(dev.err)[0]) == 0
