"""mpqe_gqe_fwd_mixed_save / mpqe_gqe_bwd_mixed / mpqe_gqe_mixed_index_build (csrc/gqe_mixed_train.h) through the C ABI,
on the host emulator and on the GPU (the `be` fixture of tests/test_gqe_kernels.py): training on queries of DIFFERENT
formulas of one query type. Problems are tests/test_gqe_mixed_kernels.py's (one set of tables and parameters that all
formulas share); every operand, block and workspace sits between fences (tests/fenced.py).

The window: runs (formula, length) = (0,1) (1,16) (2,17) (3,1) (4,1) (0,3), B = 39 -- stretches end inside, exactly at and
one past a 16-row block, formula 0 returns (its parameters get terms from two separate runs), negative lengths cycle
through 0, 1, 15, 16, 17, 33 (chain-form pair stretches cross 16 and 32), and the same anchor / the same target sits in
two queries of different formulas.

Oracles: tests/gqe_oracle.Oracle in float64 run by run without zero_grad (tolerances FWD / BWD of that file; the problems
are searched as gqe_common.settled_problem searches: the float64 oracle alone finds no near tie in any run, the float32
oracle stays within half of FWD / BWD, at most 50 seeds, so 0 queries are dropped); in the exact tests every value is an
exactly representable number (one-hot +-2^k table rows, integer parameters and score gradients, the dot score), so the
order of a sum cannot matter and scores and gradients are compared with array_equal against the float64 oracle AND
against mpqe_gqe_fwd + mpqe_gqe_bwd accumulated run by run on the same backend."""
import copy
import ctypes

import numpy as np
import pytest

from mpqe_amd import _capi
from tests import gqe_common as gc
from tests import test_gqe_mixed_kernels as mk
from tests.fenced import FILLS, assert_fence_intact, fenced, fenced_bytes
from tests.gqe_oracle import BWD, FWD, Oracle
from tests.gqe_vec_oracle import VecOracle
from tests.test_gqe_kernels import INVALID, OK, TYPES, WORKSPACE, be  # noqa: F401  (`be`: the backend fixture)

RUNS = ((0, 1), (1, 16), (2, 17), (3, 1), (4, 1), (0, 3))
C = _capi.GQE_MIX_GRAD_CHUNK
FLAG_BAD_NODE_ID, FLAG_BAD_INDEX = 1, 8
INTER_TYPES = ('2-inter', '3-inter', '3-inter_chain', '3-chain_inter')


class DotOracle(Oracle):
    """the cosine replaced by the plain dot product (programme int [27] = 1)"""

    def cos(self, a, b):
        s = (a.v * b.v).sum(1)
        return self._rec(s, (a, b), lambda g: (g[:, None] * b.v, g[:, None] * a.v))


def param_keys(P):
    """oracle key of every table and of every parameter of a Params"""
    tabs = ['enc.feat-%s.weight' % m for m in gc.MODES]
    mats = [None] * len(P.mats)
    for key, k in P.index.items():
        mats[k] = 'path_dec.' + key if not isinstance(key, tuple) else 'inter_dec.%s_%smat' % (key[1], key[0])
    return tabs, mats


def duplicate_ids(prob):
    """the same anchor and the same target in two queries of different formulas (the modes allow it: five formulas, three modes)"""
    done = set()
    for what in ('anchor', 'target'):
        for q1 in range(prob.B):
            for q2 in range(q1 + 1, prob.B):
                f1, f2 = (prob.formulas[prob.formula_of[q]] for q in (q1, q2))
                if prob.formula_of[q1] == prob.formula_of[q2] or what in done:
                    continue
                if what == 'anchor' and f1.anchor_modes[0] == f2.anchor_modes[0]:
                    prob.anchors[q2, 0] = prob.anchors[q1, 0]
                    done.add(what)
                if what == 'target' and f1.target_mode == f2.target_mode:
                    prob.targets[q2] = prob.targets[q1]
                    done.add(what)
    return done


def run_oracle(prob, cls=Oracle, dtype=np.float64, **kw):
    """-> (oracle with the gradients of all runs, scores in the layout of the whole, near ties over all runs)"""
    P = prob.params
    tabs, mats = param_keys(P)
    params = dict(zip(tabs, P.tables))
    params.update(zip(mats, P.mats))
    o = cls(params, P.node_map, dtype=dtype, **kw)
    o.flipped = getattr(prob, 'flipped', ())
    scores = np.zeros(prob.n, dtype=dtype)
    ties = 0
    for f, lo, hi in prob.runs():
        a, b = int(prob.neg_off[lo]), int(prob.neg_off[hi])
        o.current = f
        s = o.forward(prob.formulas[f], prob.anchors[lo:hi], prob.targets[lo:hi], prob.negs[a:b], prob.neg_lengths[lo:hi],
                      prob.inter)
        scores[lo:hi] = s[:hi - lo]
        scores[prob.B + a:prob.B + b] = s[hi - lo:]
        bad = np.zeros(hi - lo, dtype=bool)
        gap = o.kept.get('min_gap')
        if gap is not None:
            bad |= ((gap > 0) & (gap <= gc.TIE_TOL)).any(axis=1)
        for h in o.kept.get('preact', []):
            bad |= (np.abs(h) <= gc.TIE_TOL).any(axis=1)
        ties += int(bad.sum())
        o.backward(np.concatenate([prob.grad_scores[lo:hi], prob.grad_scores[prob.B + a:prob.B + b]]))
    return o, scores, ties


def within_half(a, b, tol):
    return bool((np.abs(a - b) <= 0.5 * (tol['atol'] + tol['rtol'] * np.abs(b))).all())


_SETTLED = {}


def settled(qt, D, inter='mean', runs=RUNS, F=5, seed=None, op='matrix', repeat=False, neg_counts=mk.NEG_COUNTS, tweak=None,
            cls=Oracle):
    """(problem, float64 oracle, its scores): the first seed from `seed` on for which the float64 oracle alone finds no near
    tie in any run and its float32 twin stays within half of FWD / BWD. Computed once, shared by both backends."""
    key = (qt, D, inter, runs, F, seed, op, repeat, neg_counts, tweak, cls)
    if key in _SETTLED:
        return _SETTLED[key]
    first = 100 * TYPES.index(qt) + D if seed is None else seed
    chain = 'inter' not in qt
    kw = {}
    if op != 'matrix':
        cls, kw = VecOracle, dict(decoder={'translate': 'transe', 'scale': 'bilinear-diag'}[op])
    for s in range(first, first + 50):
        prob = mk.Problem(qt, D, F, runs, s, op=op, inter=inter, repeat=repeat, neg_counts=neg_counts,
                          score='dot' if op == 'scale' and chain else 'cosine')
        if runs == RUNS:
            assert duplicate_ids(prob) == {'anchor', 'target'}
        if tweak is not None:
            tweak(prob)
        prob.grad_scores = np.random.RandomState(s + 7).normal(0, 1.0, prob.n).astype(np.float32)
        o, scores, ties = run_oracle(prob, cls, **kw)
        if ties:
            continue
        o32, s32, _ = run_oracle(prob, cls, dtype=np.float32, **kw)
        if within_half(s32, scores, FWD) and all(within_half(o32.grads[k], o.grads[k], BWD) for k in o.grads):
            _SETTLED[key] = (prob, o, scores)
            return _SETTLED[key]
    raise AssertionError('no seed without near-ties')


def exact_problem(qt, inter, runs=RUNS, F=5, seed=3, neg_counts=mk.NEG_COUNTS):
    """one-hot +-2^k table rows, integer parameters and score gradients in -2..2, the dot score, the matrix operator, D 16"""
    key = ('exact', qt, inter, runs, F, seed, neg_counts)
    if key in _SETTLED:
        return _SETTLED[key]
    prob = mk.Problem(qt, 16, F, runs, seed, inter=inter, neg_counts=neg_counts)
    rng = np.random.RandomState(seed + 11)
    P = prob.params
    for t in P.tables:
        t[...] = 0
        rows = np.arange(t.shape[0])
        t[rows, rng.randint(0, 16, size=t.shape[0])] = rng.choice([-1.0, 1.0], size=t.shape[0]) * 2.0 ** rng.randint(-2, 3, size=t.shape[0])
    for m in P.mats:
        m[...] = rng.randint(-2, 3, size=m.shape)
    prob.progs[:, 27] = 1
    if runs == RUNS:
        duplicate_ids(prob)
    prob.grad_scores = rng.randint(-2, 3, size=prob.n).astype(np.float32)
    o, scores, _ = run_oracle(prob, DotOracle)
    _SETTLED[key] = (prob, o, scores)
    return _SETTLED[key]


class Train(mk.Device):
    """A problem's shared operands on a backend plus the index block, the training workspace and the three calls."""

    def __init__(self, be, prob):
        super(Train, self).__init__(be, prob)
        self.T, self.M = len(self.tables), len(self.mats)
        self.nm = int(self.node_map.shape[0])

    def build_index(self, fill='nan', short=0, progs=None):
        be, prob = self.be, self.prob
        progs = np.ascontiguousarray(prob.progs if progs is None else progs, dtype=np.int32)
        self.index_bytes = be.lib.mpqe_gqe_mixed_index_bytes(progs.shape[0])
        assert self.index_bytes > 0
        self.index = fenced_bytes(be, self.index_bytes - short, fill)
        return be.lib.mpqe_gqe_mixed_index_build(progs.ctypes.data, progs.shape[0], self.T, self.M, prob.D,
                                                 be.ptr(self.index), self.index_bytes - short, be.stream)

    def ready(self):
        assert self.build() == OK and self.build_index() == OK
        return self

    def place(self, win=None, formula_of=None, fill='nan', short=0, F=None):
        """the operands of window `win` (a Problem-like; default: the problem) and a workspace holding `fill`"""
        be = self.be
        win = self.win = self.prob if win is None else win
        p_ids, e_ids, qrow, neg_off, n = win.operands(0, win.B)
        self.n, self.p_rows, self.e_rows = n, p_ids.shape[1], e_ids.shape[0]
        self.keep = [mk.place(be, p_ids), mk.place(be, e_ids), None if qrow is None else mk.place(be, qrow),
                     None if neg_off is None else mk.place(be, neg_off),
                     mk.place(be, win.formula_of if formula_of is None else formula_of)]
        self.scores = mk.place(be, np.full(n, np.float32(7.5)))
        self.prog = np.ascontiguousarray(win.progs[0])
        self.F = win.F if F is None else F
        self.wb = be.lib.mpqe_gqe_mixed_train_workspace_bytes(self.prog.ctypes.data, self.F, self.T, self.M, self.p_rows, n,
                                                              win.D) if win.B else 256
        assert self.wb > 0
        self.ws = fenced_bytes(be, self.wb - short, fill)
        self.short = short
        self.gs = mk.place(be, win.grad_scores)
        self.gtabs = [fenced(be, np.zeros(tuple(t.shape), np.float32)) for t in self.tables]
        self.gmats = [fenced(be, np.zeros(tuple(m.shape), np.float32)) for m in self.mats]
        return self

    def _window(self):
        be, k = self.be, self.keep
        return (be.ptr(self.node_map), self.nm, self.win.D, be.ptr(k[4]), self.win.B, be.ptr(k[0]), self.p_rows, be.ptr(k[1]),
                self.e_rows, be.ptr(k[2]), be.ptr(k[3]), self.n, 1e-8)

    def forward(self, ws_ptr=None):
        be = self.be
        head = (self.prog.ctypes.data, self.F, be.ptr(self.desc), self.desc_bytes, self.T, self.M)
        return be.lib.mpqe_gqe_fwd_mixed_save(*(head + self._window() + (
            be.ptr(self.scores), be.ptr(self.ws) if ws_ptr is None else ws_ptr, self.wb - self.short, be.ptr(self.err),
            be.stream)))

    def forward_plain(self):
        be = self.be
        scores = mk.place(be, np.full(self.n, np.float32(7.5)))
        head = (self.prog.ctypes.data, self.F, be.ptr(self.desc), self.desc_bytes)
        st = be.lib.mpqe_gqe_fwd_mixed(*(head + self._window() + (be.ptr(scores), be.ptr(self.err), be.stream)))
        return st, scores

    def backward(self, null_tabs=(), null_mats=(), ws_ptr=None, index_short=0):
        be = self.be
        gt = (ctypes.c_void_p * self.T)(*[None if t in null_tabs else be.ptr(g) for t, g in enumerate(self.gtabs)])
        gm = (ctypes.c_void_p * self.M)(*[None if m in null_mats else be.ptr(g) for m, g in enumerate(self.gmats)])
        head = (self.prog.ctypes.data, self.F, be.ptr(self.desc), self.desc_bytes, be.ptr(self.index),
                self.index_bytes - index_short, self.T, self.M)
        return be.lib.mpqe_gqe_bwd_mixed(*(head + self._window() + (
            be.ptr(self.gs), gt, gm, be.ptr(self.ws) if ws_ptr is None else ws_ptr, self.wb - self.short, be.ptr(self.err),
            be.stream)))

    def grads(self):
        """{oracle key: array}; every fence and every table's padding row checked on the way"""
        be = self.be
        tabs, mats = param_keys(self.prob.params)
        out = {}
        for k, g in list(zip(tabs, self.gtabs)) + list(zip(mats, self.gmats)):
            assert_fence_intact(be, g, 'grad ' + k)
            out[k] = be.get(g).copy()
        for k in tabs:
            assert not out[k][-1].any(), 'padding row of ' + k
        for what in ('ws', 'desc', 'index'):
            assert_fence_intact(be, getattr(self, what), what)
        if self.win.B:                                  # (an empty operand is a plain array: mk.place)
            for t in [self.scores, self.gs] + [k for k in self.keep if k is not None]:
                assert_fence_intact(be, t, 'operand')
        for t in self.tables + self.mats + [self.node_map]:
            assert_fence_intact(be, t, 'operand')
        return out

    def run(self, win=None, **kw):
        """forward with states + backward -> (scores, gradients)"""
        self.place(win, **kw)
        assert self.forward() == OK
        assert self.backward() == OK
        return self.be.get(self.scores).copy(), self.grads()

    def per_formula_train(self):
        """mpqe_gqe_fwd(save_states = 1) + mpqe_gqe_bwd run by run, the gradients accumulating in one set of buffers"""
        be, prob = self.be, self.prob
        scores = np.zeros(prob.n, dtype=np.float32)
        gtabs = [be.zeros(tuple(t.shape), np.float32) for t in self.tables]
        gmats = [be.zeros(tuple(m.shape), np.float32) for m in self.mats]
        gt = (ctypes.c_void_p * self.T)(*[be.ptr(g) for g in gtabs])
        gm = (ctypes.c_void_p * self.M)(*[be.ptr(g) for g in gmats])
        for f, lo, hi in prob.runs():
            p_ids, e_ids, qrow, neg_off, n = prob.operands(lo, hi)
            a, b = int(prob.neg_off[lo]), int(prob.neg_off[hi])
            keep = [be.put(p_ids), be.put(e_ids), None if qrow is None else be.put(qrow),
                    None if neg_off is None else be.put(neg_off),
                    be.put(np.concatenate([prob.grad_scores[lo:hi], prob.grad_scores[prob.B + a:prob.B + b]]))]
            out = be.empty((n,), np.float32)
            prog = np.ascontiguousarray(prob.progs[f])
            wb = be.lib.mpqe_gqe_workspace_bytes(prog.ctypes.data, p_ids.shape[1], n, prob.D)
            ws = be.nbytes(wb + 256)
            wp = (be.ptr(ws) + 255) // 256 * 256
            common = (prog.ctypes.data, self.tab, self.rows, self.T, be.ptr(self.node_map), self.nm, self.mat, self.M, prob.D,
                      be.ptr(keep[0]), p_ids.shape[1], be.ptr(keep[1]), e_ids.shape[0], be.ptr(keep[2]), be.ptr(keep[3]), n,
                      1e-8)
            assert be.lib.mpqe_gqe_fwd(*(common + (1, be.ptr(out), wp, wb, be.ptr(self.err), be.stream))) == OK
            assert be.lib.mpqe_gqe_bwd(*(common + (be.ptr(keep[4]), gt, gm, wp, wb, be.ptr(self.err), be.stream))) == OK
            got = be.get(out)
            scores[lo:hi] = got[:hi - lo]
            scores[prob.B + a:prob.B + b] = got[hi - lo:]
        tabs, mats = param_keys(prob.params)
        return scores, {k: be.get(g) for k, g in list(zip(tabs, gtabs)) + list(zip(mats, gmats))}


def assert_close(prob, o, want, scores, grads):
    np.testing.assert_allclose(scores, want, **FWD)
    for k, g in grads.items():
        print('%s: max abs error %.3g (max |ref| %.3g)' % (k, np.abs(g - o.grads[k]).max(), np.abs(o.grads[k]).max()))
        np.testing.assert_allclose(g, o.grads[k], err_msg=k, **BWD)
    assert any(g.any() for k, g in grads.items() if k.startswith('enc.'))
    assert any(g.any() for k, g in grads.items() if not k.startswith('enc.'))


def assert_same_bits(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        np.testing.assert_array_equal(mk.bits(a[k]), mk.bits(b[k]), err_msg=k)


def _main_cases():
    out = []
    for qt in TYPES:
        for inter in (('mean', 'min') if qt in INTER_TYPES else ('mean',)):
            for D in (16, 48, 128, 256):
                out.append((qt, inter, D))
    return out


# ---------------------------------------------------------------------------------------------- 1 and 3
@pytest.mark.parametrize('qt,inter,D', _main_cases())
def test_against_float64_and_forward_bits(be, qt, inter, D):
    prob, o, want = settled(qt, D, inter)
    assert prob.B == 39 and sorted(set(prob.neg_lengths)) == sorted(mk.NEG_COUNTS) and len(prob.runs()) == 6
    dev = Train(be, prob).ready()
    scores, grads = dev.run()
    assert int(be.get(dev.err)[0]) == 0
    assert_close(prob, o, want, scores, grads)
    # the scores of the forward with states are the plain mixed forward's, bit for bit
    st, plain = dev.forward_plain()
    assert st == OK
    np.testing.assert_array_equal(mk.bits(scores), mk.bits(be.get(plain)))


# ---------------------------------------------------------------------------------------------- 2
EXACT = [('2-chain', 'mean'), ('3-chain', 'mean'), ('2-inter', 'mean'), ('2-inter', 'min'), ('3-inter', 'min'),
         ('3-inter_chain', 'min')]


def check_exact(be, prob, o, want):
    dev = Train(be, prob).ready()
    scores, grads = dev.run()
    assert int(be.get(dev.err)[0]) == 0
    ref_scores, ref_grads = dev.per_formula_train()
    assert max(np.abs(g).max() for g in grads.values()) > 1
    np.testing.assert_array_equal(scores, want.astype(np.float32))
    np.testing.assert_array_equal(scores, ref_scores)
    for k, g in grads.items():
        np.testing.assert_array_equal(g, o.grads[k].astype(np.float32), err_msg=k)
        np.testing.assert_array_equal(g, ref_grads[k], err_msg=k)


@pytest.mark.parametrize('qt,inter', EXACT)
def test_exact_arithmetic(be, qt, inter):
    prob, o, want = exact_problem(qt, inter)
    assert prob.progs[0][27] == 1 and (qt not in INTER_TYPES or prob.progs[0][3] >= 0)
    check_exact(be, prob, o, want)


# ---------------------------------------------------------------------------------------------- 4
def _one_parameter(prob):
    """every formula becomes formula 0: one parameter per site"""
    prob.progs[:] = prob.progs[0]
    prob.formulas = [prob.formulas[0]] * prob.F
    prob.plans = [prob.plans[0]] * prob.F


@pytest.mark.parametrize('count', [C - 1, C, C + 1, 2 * C + 1])
@pytest.mark.parametrize('exact', [False, True])
def test_one_parameter_at_the_chunk_edges(be, count, exact):
    """a 1-chain with no negatives has one site and one P row per query: `count` queries of one formula (in two runs, so that
    the window is not one run) give that formula's matrix exactly `count` contributions"""
    runs = ((0, count - 3), (1, 3))
    if exact:
        # (formula 1 gets formula 0's programme: one matrix, `count` contributions)
        key = ('edge', count)
        if key not in _SETTLED:
            prob, o, want = exact_problem('1-chain', 'mean', runs, 2, 5, (0,))
            prob = copy.deepcopy(prob)
            _one_parameter(prob)
            o, want, _ = run_oracle(prob, DotOracle)
            _SETTLED[key] = (prob, o, want)
        prob, o, want = _SETTLED[key]
        assert prob.n == prob.B == count
        check_exact(be, prob, o, want)
        return
    prob, o, want = settled('1-chain', 16, runs=runs, F=2, seed=5, neg_counts=(0,), tweak=_one_parameter)
    assert prob.n == prob.B == count and len({tuple(p) for p in prob.progs}) == 1
    scores, grads = Train(be, prob).ready().run()
    assert_close(prob, o, want, scores, grads)
    assert sum(1 for k, g in grads.items() if k.startswith('path_dec.') and g.any()) == 1


@pytest.mark.parametrize('qt', ['2-chain', '3-inter'])
@pytest.mark.parametrize('exact', [False, True])
def test_every_query_a_formula_of_its_own(be, qt, exact):
    runs = tuple((f, 1) for f in range(33))
    if exact:
        prob, o, want = exact_problem(qt, 'min', runs, 33, 11, (0, 1, 17))
        assert prob.B == prob.F == 33
        return check_exact(be, prob, o, want)
    prob, o, want = settled(qt, 48, 'min' if qt == '3-inter' else 'mean', runs=runs, F=33, seed=11, neg_counts=(0, 1, 17))
    assert prob.B == prob.F == 33
    scores, grads = Train(be, prob).ready().run()
    assert_close(prob, o, want, scores, grads)


class FlipOracle(Oracle):
    """the path matrices of the formulas in `flipped` are used the other way round (a raw programme's code ^ 1)"""
    flipped, current = (), None

    def mm(self, x, key, transposed):
        if key.startswith('path_dec.') and self.current in self.flipped:
            transposed = not transposed
        return super(FlipOracle, self).mm(x, key, transposed)


def test_one_matrix_plain_and_transposed_in_one_window(be):
    """a raw programme: formula 1 is formula 0 with the transposition bit of its one site flipped -- the same matrix, used
    as M by one formula and as M^T by the other in the same window (and in the same chunk of its contributions)"""
    def tweak(prob):
        prob.formulas[1], prob.plans[1] = prob.formulas[0], prob.plans[0]
        prob.progs[1] = prob.progs[0]
        prob.progs[1][10] ^= 1
        prob.flipped = (1,)
    prob, o, want = settled('1-chain', 48, runs=((0, 5), (1, 17), (0, 1)), F=2, seed=81, tweak=tweak, cls=FlipOracle)
    assert prob.progs[0][10] >> 1 == prob.progs[1][10] >> 1 and prob.progs[0][10] & 1 != prob.progs[1][10] & 1
    scores, grads = Train(be, prob).ready().run()
    assert_close(prob, o, want, scores, grads)


@pytest.mark.parametrize('qt', ['2-chain', '2-inter'])
def test_one_relation_at_two_sites(be, qt):
    """r.r / r & r (formula 0) next to a formula that uses the relation once (formula 1: its second relation replaced)"""
    def tweak(prob):
        from mpqe_amd.graph import Formula
        from mpqe_amd.model import gqe_plan
        r = prob.formulas[0].rels[0]
        other = (r[0], [n for n in gc.NAMES if n != r[1]][0], r[2])
        prob.formulas[1] = Formula(qt, (r, other))
        prob.plans = [gqe_plan(f) for f in prob.formulas]
        prob.progs = np.stack([prob.params.programme(f, prob.inter, 'cosine') for f in prob.formulas]).astype(np.int32)
    prob, o, want = settled(qt, 48, 'min' if qt == '2-inter' else 'mean', runs=((0, 5), (1, 17), (0, 1)), F=2, seed=71,
                            repeat=True, tweak=tweak)
    assert prob.formulas[0].rels[0] == prob.formulas[0].rels[1] and prob.formulas[1].rels[0] != prob.formulas[1].rels[1]
    scores, grads = Train(be, prob).ready().run()
    assert_close(prob, o, want, scores, grads)


@pytest.mark.parametrize('qt', ['3-chain', '3-inter_chain'])
@pytest.mark.parametrize('op', ['translate', 'scale'])
def test_vector_operators(be, qt, op):
    prob, o, want = settled(qt, 48, seed=41 + TYPES.index(qt), op=op)
    assert prob.progs[0][7] == {'translate': 1, 'scale': 2}[op]
    assert qt != '3-inter_chain' or prob.progs[0][3] >= 0            # (pre / post stay matrices)
    scores, grads = Train(be, prob).ready().run()
    assert_close(prob, o, want, scores, grads)
    assert any(g.ndim == 1 and g.any() for g in grads.values())


# ---------------------------------------------------------------------------------------------- 5
def test_bits_do_not_depend_on_the_run_or_the_workspace(be):
    """the same window again, and again with the workspace pre-filled with each of fenced.FILLS: the same score and
    gradient bits. (Nothing is asserted across a permutation of the window: the window defines the order of the sums.)"""
    prob, o, want = settled('3-inter_chain', 48, 'min')
    dev = Train(be, prob).ready()
    first = dev.run()
    for fill in sorted(FILLS):
        scores, grads = dev.run(fill=fill)
        assert scores.tobytes() == first[0].tobytes(), fill
        assert_same_bits(grads, first[1])


# ---------------------------------------------------------------------------------------------- 6
def without(prob, victim):
    """the window with one query removed"""
    w = copy.copy(prob)
    keep = np.arange(prob.B) != victim
    pair_keep = np.concatenate([keep, np.repeat(keep, prob.neg_lengths)])
    a, b = int(prob.neg_off[victim]), int(prob.neg_off[victim + 1])
    w.formula_of, w.anchors, w.targets = prob.formula_of[keep], prob.anchors[keep], prob.targets[keep]
    w.neg_lengths = prob.neg_lengths[keep]
    w.negs = np.concatenate([prob.negs[:a], prob.negs[b:]])
    w.neg_off = np.concatenate([[0], np.cumsum(w.neg_lengths)]).astype(np.int64)
    w.grad_scores = prob.grad_scores[pair_keep]
    w.B, w.n = prob.B - 1, int(pair_keep.sum())
    return w, pair_keep


@pytest.mark.parametrize('bad', [-1, 5, 2 ** 40])
@pytest.mark.parametrize('qt', ['2-chain', '3-inter'])
def test_bad_formula_index_and_bad_anchor(be, qt, bad):
    """Query 21 (inside the run of 17) has a formula index out of range: MPQE_FLAG_BAD_INDEX, its pairs score 0 and every
    gradient is BIT FOR BIT that of the window without it. Query 30 has an anchor of no mode in both windows (its row is
    zeros and gets no table gradient; it still takes part in the other sums, so it cannot be compared with its removal)."""
    prob, o, want = settled(qt, 48, 'mean')
    victim, sick = 21, 30
    win = copy.copy(prob)
    win.anchors = prob.anchors.copy()
    win.anchors[sick, 0] = prob.params.node_map.shape[0] - 1          # (in the map, of no mode: -1)
    fo = prob.formula_of.copy()
    fo[victim] = bad
    dev = Train(be, prob).ready()
    scores, grads = dev.run(win, formula_of=fo)
    assert int(be.get(dev.err)[0]) == FLAG_BAD_INDEX | FLAG_BAD_NODE_ID
    dev.err = be.zeros(1, np.int32)
    less, pair_keep = without(win, victim)
    ref_scores, ref_grads = dev.run(less)
    assert int(be.get(dev.err)[0]) == FLAG_BAD_NODE_ID
    np.testing.assert_array_equal(mk.bits(scores[pair_keep]), mk.bits(ref_scores))
    assert (scores[~pair_keep] == 0).all()
    assert_same_bits(grads, ref_grads)
    assert all(np.isfinite(g).all() for g in grads.values())
    # the healthy window differs (the victim's and the sick query's terms are in it)
    clean = dev.run()[1]
    assert any(clean[k].tobytes() != grads[k].tobytes() for k in clean)


def test_null_gradient_entries_are_neither_computed_nor_written(be):
    prob, o, want = settled('3-inter', 48, 'mean')
    dev = Train(be, prob).ready()
    _, full = dev.run()
    tabs, mats = param_keys(prob.params)
    used = [m for m, k in enumerate(mats) if full[k].any()]
    null_mats, null_tabs = set(used[::2]), {t for t, k in enumerate(tabs) if full[k].any()}
    null_tabs = set(sorted(null_tabs)[:1])
    dev.place()
    assert dev.forward() == OK and dev.backward(null_tabs=null_tabs, null_mats=null_mats) == OK
    got = dev.grads()
    for t, k in enumerate(tabs):
        np.testing.assert_array_equal(mk.bits(got[k]), mk.bits(np.zeros_like(full[k]) if t in null_tabs else full[k]), err_msg=k)
    for m, k in enumerate(mats):
        np.testing.assert_array_equal(mk.bits(got[k]), mk.bits(np.zeros_like(full[k]) if m in null_mats else full[k]), err_msg=k)


def test_gradients_are_added(be):
    prob, o, want = settled('2-chain', 16)
    dev = Train(be, prob).ready()
    _, once = dev.run()
    assert dev.backward() == OK                      # (the same buffers again)
    twice = dev.grads()
    for k in once:
        np.testing.assert_array_equal(twice[k], once[k] + once[k], err_msg=k)


@pytest.mark.parametrize('fill', ['zeros', 'noise'])
def test_blocks_and_workspace_are_exactly_their_declared_size(be, fill):
    prob, o, want = settled('3-inter', 48, 'mean')
    dev = Train(be, prob).ready()
    _, full = dev.run()
    # the index block: one byte short is refused by the build with nothing written, and by the backward
    assert dev.build_index(fill=fill, short=1) == WORKSPACE
    np.testing.assert_array_equal(be.get(dev.index), np.resize(FILLS[fill], dev.index_bytes - 1))
    assert_fence_intact(be, dev.index, 'index')
    assert be.lib.mpqe_gqe_mixed_index_bytes(0) == 0
    assert dev.build_index(fill=fill) == OK
    assert_fence_intact(be, dev.index, 'index')
    dev.place(fill=fill)
    assert dev.forward() == OK
    assert dev.backward(index_short=1) == WORKSPACE
    # the workspace: one byte short is refused by both calls with nothing written; not 256-aligned is an invalid argument
    dev.place(fill=fill, short=1)
    assert dev.forward() == WORKSPACE and dev.backward() == WORKSPACE
    np.testing.assert_array_equal(be.get(dev.ws), np.resize(FILLS[fill], dev.wb - 1))
    assert (be.get(dev.scores) == np.float32(7.5)).all()
    assert not any(g.any() for g in dev.grads().values())
    dev.place(fill=fill)
    assert dev.forward(ws_ptr=be.ptr(dev.ws) + 16) == INVALID and dev.backward(ws_ptr=be.ptr(dev.ws) + 16) == INVALID
    np.testing.assert_array_equal(be.get(dev.ws), np.resize(FILLS[fill], dev.wb))
    # exact: the whole pass in a workspace of the declared size, fenced (Train.grads checks the fences)
    assert dev.forward() == OK and dev.backward() == OK
    assert_same_bits(dev.grads(), full)
    assert be.lib.mpqe_gqe_mixed_train_workspace_bytes(dev.prog.ctypes.data, 0, dev.T, dev.M, 39, dev.n, 48) == 0
    assert be.lib.mpqe_gqe_mixed_train_workspace_bytes(dev.prog.ctypes.data, 5, dev.T, dev.M, 39, dev.n, 40) == 0


def test_index_build_refuses_programmes_that_disagree(be):
    prob = mk.problem('2-inter', 48, 3, mk.RUNS_MAIN, 100 * TYPES.index('2-inter') + 48)
    other = mk.problem('3-inter', 48, 3, mk.RUNS_MAIN, 100 * TYPES.index('3-inter') + 48).progs[1]
    agg = prob.progs[1].copy()
    agg[2] = 1
    dev = Train(be, prob)
    for bad in (other, agg):
        progs = prob.progs.copy()
        progs[2] = bad
        assert dev.build_index(fill='noise', progs=progs) == INVALID
        np.testing.assert_array_equal(be.get(dev.index), np.resize(FILLS['noise'], dev.index_bytes))
        assert_fence_intact(be, dev.index, 'index')


@pytest.mark.parametrize('qt', ['1-chain', '2-inter'])
def test_no_queries(be, qt):
    prob = mk.Problem(qt, 48, 2, (), 31)
    prob.grad_scores = np.zeros(0, dtype=np.float32)
    dev = Train(be, prob).ready()
    dev.place()
    assert dev.forward() == OK and dev.backward() == OK and int(be.get(dev.err)[0]) == 0
    assert not any(g.any() for g in dev.grads().values())
