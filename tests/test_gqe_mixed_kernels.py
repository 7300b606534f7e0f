"""mpqe_gqe_fwd_mixed / mpqe_gqe_mixed_desc_build (csrc/gqe.hip) through the C ABI, on the host emulator and on the GPU
(the `be` fixture of tests/test_gqe_kernels.py): queries of DIFFERENT formulas of one query type scored in one launch.

The oracle is mpqe_gqe_fwd on the same backend, handed every run of equal formula alone with its own programme; the
scores are compared as uint32 BITS (the contract of include/mpqe_amd.h: no tolerance). Problems are built from
tests/gqe_common.py's pieces (its modes, relation names, formula generator and node map) over ONE set of tables and
parameters that all formulas share. Every operand sits between fences (tests/fenced.py): a read outside an id list meets
the integer fence (no id: the error word is set, which every clean case asserts it is not), a read outside a table or a
matrix meets a NaN, a write outside the scores or the descriptor block is caught bit for bit.

Shapes: D 16 / 48 (lanes past D) / 256; all seven query types; run lengths 1, 16, 17 (a stretch that ends inside, exactly
at and one past a 16-row block); negative counts 0, 1, 15, 16, 17, 33 per query, so that the chain form's stretches of
pair rows end at, one short of and one past 16 and 32 rows."""
import ctypes

import numpy as np
import pytest

from tests import gqe_common as gc
from tests.fenced import FILLS, assert_fence_intact, fenced, fenced_bytes
from tests.test_gqe_kernels import INVALID, OK, TYPES, WORKSPACE, be  # noqa: F401  (`be`: the backend fixture)

ROWS = 23
NEG_COUNTS = (0, 1, 15, 16, 17, 33)
RUNS_MAIN = ((0, 1), (1, 16), (2, 17))          # (formula, run length)
FLAG_BAD_NODE_ID, FLAG_BAD_INDEX = 1, 8


def relation_keys():
    return ['%s_%s_%s' % (a, name, b) for a in gc.MODES for name in gc.NAMES for b in gc.MODES]


class Params(object):
    """The tables and parameters every formula of a problem shares, numbered once: table t = mode gc.MODES[t]; parameter
    k = relation relation_keys()[k] (a [D, D] matrix, or a [D] vector under a vector operator), then the pre and the post
    matrix of every mode."""

    def __init__(self, D, op, seed):
        rng = np.random.RandomState(seed)
        self.D, self.op = D, op
        n_ent = ROWS * len(gc.MODES)
        self.node_map = np.full(n_ent + 1, -1, dtype=np.int64)
        self.ids = {}
        for k, mode in enumerate(gc.MODES):
            self.ids[mode] = np.arange(k, n_ent, len(gc.MODES), dtype=np.int64)
            self.node_map[self.ids[mode]] = np.arange(ROWS)
        self.tables = [rng.normal(0, 1.0, (ROWS + 1, D)).astype(np.float32) for _ in gc.MODES]
        lim = np.sqrt(6.0 / (2 * D))
        self.mats, self.index = [], {}
        for key in relation_keys():
            self.index[key] = len(self.mats)
            if op == 'matrix':
                self.mats.append(rng.uniform(-lim, lim, (D, D)).astype(np.float32))
            elif op == 'translate':
                self.mats.append(rng.uniform(-lim, lim, (D,)).astype(np.float32))
            else:
                self.mats.append(rng.uniform(0.5, 1.5, (D,)).astype(np.float32))
        for mode in gc.MODES:
            for which in ('pre', 'post'):
                self.index[(which, mode)] = len(self.mats)
                self.mats.append(rng.uniform(-lim, lim, (D, D)).astype(np.float32))

    def programme(self, formula, inter, score):
        from mpqe_amd import ops
        from mpqe_amd.model import gqe_plan
        form, branches, imode, tail, emode = gqe_plan(formula)
        t = gc.MODES.index
        pb = [(t(m), [(self.index['_'.join(r)], tr) for r, tr in steps]) for _, m, steps in branches]
        pt = [(self.index['_'.join(r)], tr) for r, tr in tail]
        pre = post = -1
        if imode is not None and not inter.endswith('simple'):
            pre, post = self.index[('pre', imode)], self.index[('post', imode)]
        return ops.gqe_programme(form, pb, t(emode), inter.split('-')[0], pre, post, pt, op=self.op,
                                 score=score if form == 0 else 'cosine')


class Problem(object):
    """B queries of one query type under F formulas: query q has formula formula_of[q]; ids drawn from the modes its formula
    names, NEG_COUNTS negatives cycling from query to query."""

    def __init__(self, qt, D, F, runs, seed, op='matrix', score='cosine', inter='mean', repeat=False, neg_counts=NEG_COUNTS):
        from mpqe_amd.model import gqe_plan
        rng = np.random.RandomState(seed)
        self.params = Params(D, op, seed + 1)
        self.qt, self.D, self.F, self.inter = qt, D, F, inter
        self.formulas = []
        while len(self.formulas) < F:
            f = gc.make_formula(qt, rng, repeat)
            if repeat or F > 18 or f not in self.formulas:       # (different formulas where there are enough to draw)
                self.formulas.append(f)
        self.progs = np.stack([self.params.programme(f, inter, score) for f in self.formulas]).astype(np.int32)
        self.plans = [gqe_plan(f) for f in self.formulas]
        self.form = self.plans[0][0]
        self.formula_of = np.concatenate([np.full(k, f, dtype=np.int64) for f, k in runs] + [np.zeros(0, dtype=np.int64)])
        B = self.B = int(self.formula_of.shape[0])
        A = len(self.formulas[0].anchor_modes)
        ids = self.params.ids
        self.anchors = np.zeros((B, A), dtype=np.int64)
        self.targets = np.zeros(B, dtype=np.int64)
        self.neg_lengths = np.array([neg_counts[q % len(neg_counts)] for q in range(B)], dtype=np.int64)
        negs = []
        for q in range(B):
            f = self.formulas[self.formula_of[q]]
            self.anchors[q] = [rng.choice(ids[m]) for m in f.anchor_modes]
            self.targets[q] = rng.choice(ids[f.target_mode])
            negs.append(rng.choice(ids[f.target_mode], size=int(self.neg_lengths[q])))
        self.negs = np.concatenate(negs + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
        self.neg_off = np.concatenate([[0], np.cumsum(self.neg_lengths)]).astype(np.int64)
        self.n = B + int(self.negs.shape[0])

    def operands(self, lo, hi):
        """(p_ids, e_ids, qrow, neg_off, n) of queries [lo, hi) alone, in mpqe_gqe_fwd's layout"""
        form, branches = self.plans[0][0], self.plans[0][1]
        a, b = int(self.neg_off[lo]), int(self.neg_off[hi])
        B = hi - lo
        tnodes = np.concatenate([self.targets[lo:hi], self.negs[a:b]]).astype(np.int64)
        lengths = self.neg_lengths[lo:hi]
        if form == 0:
            qrow = np.concatenate([np.arange(B), np.repeat(np.arange(B), lengths)]).astype(np.int64)
            return tnodes.reshape(1, -1), self.anchors[lo:hi, 0].copy(), qrow, None, tnodes.shape[0]
        p_ids = np.ascontiguousarray(np.stack([self.anchors[lo:hi, slot] for slot, _, _ in branches]))
        return p_ids, tnodes, None, (self.neg_off[lo:hi + 1] - a).astype(np.int64), tnodes.shape[0]

    def runs(self):
        from mpqe_amd.model import formula_runs
        return formula_runs(self.formula_of)


class Device(object):
    """A problem's shared operands on a backend, fenced, and the two calls."""

    def __init__(self, be, prob):
        self.be, self.prob = be, prob
        P = prob.params
        self.tables = [fenced(be, t) for t in P.tables]
        self.mats = [fenced(be, m) for m in P.mats]
        self.node_map = fenced(be, P.node_map)
        self.tab = (ctypes.c_void_p * len(self.tables))(*[be.ptr(t) for t in self.tables])
        self.rows = (ctypes.c_int64 * len(self.tables))(*[int(t.shape[0]) for t in self.tables])
        self.mat = (ctypes.c_void_p * len(self.mats))(*[be.ptr(m) for m in self.mats])
        self.err = be.zeros(1, np.int32)

    def per_formula(self):
        """the oracle: every run through mpqe_gqe_fwd with its own programme -> scores in the layout of the whole"""
        be, prob = self.be, self.prob
        out = np.zeros(prob.n, dtype=np.float32)
        for f, lo, hi in prob.runs():
            p_ids, e_ids, qrow, neg_off, n = prob.operands(lo, hi)
            keep = [be.put(p_ids), be.put(e_ids), None if qrow is None else be.put(qrow),
                    None if neg_off is None else be.put(neg_off)]
            scores = be.empty((n,), np.float32)
            prog = np.ascontiguousarray(prob.progs[f])
            st = be.lib.mpqe_gqe_fwd(prog.ctypes.data, self.tab, self.rows, len(self.tables), be.ptr(self.node_map),
                                     int(self.node_map.shape[0]), self.mat, len(self.mats), prob.D, be.ptr(keep[0]),
                                     p_ids.shape[1], be.ptr(keep[1]), e_ids.shape[0], be.ptr(keep[2]), be.ptr(keep[3]), n,
                                     1e-8, 0, be.ptr(scores), None, 0, be.ptr(self.err), be.stream)
            assert st == OK
            got = be.get(scores)
            a, b = int(prob.neg_off[lo]), int(prob.neg_off[hi])
            out[lo:hi] = got[:hi - lo]
            out[prob.B + a:prob.B + b] = got[hi - lo:]
        return out

    def build(self, fill='nan', short=0, progs=None):
        be, prob = self.be, self.prob
        progs = np.ascontiguousarray(prob.progs if progs is None else progs, dtype=np.int32)
        self.desc_bytes = be.lib.mpqe_gqe_mixed_desc_bytes(progs.shape[0])
        assert self.desc_bytes > 0
        self.desc = fenced_bytes(be, self.desc_bytes - short, fill)
        return be.lib.mpqe_gqe_mixed_desc_build(progs.ctypes.data, progs.shape[0], self.tab, self.rows, len(self.tables),
                                                self.mat, len(self.mats), prob.D, be.ptr(self.desc), self.desc_bytes - short,
                                                be.stream)

    def mixed(self, formula_of=None, anchors=None, targets=None, F=None, short=0):
        """-> (status, scores view); the whole problem in one mpqe_gqe_fwd_mixed call"""
        be, prob = self.be, self.prob
        saved = prob.anchors, prob.targets
        if anchors is not None:
            prob.anchors = anchors
        if targets is not None:
            prob.targets = targets
        p_ids, e_ids, qrow, neg_off, n = prob.operands(0, prob.B)
        prob.anchors, prob.targets = saved
        fo = place(be, prob.formula_of if formula_of is None else formula_of)
        self.keep = [place(be, p_ids), place(be, e_ids), None if qrow is None else place(be, qrow),
                     None if neg_off is None else place(be, neg_off), fo]
        scores = place(be, np.full(n, np.float32(7.5)))
        prog = np.ascontiguousarray(prob.progs[0])
        st = be.lib.mpqe_gqe_fwd_mixed(prog.ctypes.data, prob.F if F is None else F, be.ptr(self.desc),
                                       self.desc_bytes - short, be.ptr(self.node_map), int(self.node_map.shape[0]), prob.D,
                                       be.ptr(fo), prob.B, be.ptr(self.keep[0]), p_ids.shape[1], be.ptr(self.keep[1]),
                                       e_ids.shape[0], be.ptr(self.keep[2]), be.ptr(self.keep[3]), n, 1e-8, be.ptr(scores),
                                       be.ptr(self.err), be.stream)
        return st, scores


def place(be, a):
    """fenced(); an empty operand (whose view would forget its address) is a plain empty array"""
    return fenced(be, a) if a.size else be.put(a)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check(be, prob):
    dev = Device(be, prob)
    want = dev.per_formula()
    assert dev.build() == OK
    st, scores = dev.mixed()
    assert st == OK
    got = be.get(scores)
    assert int(be.get(dev.err)[0]) == 0
    assert np.isfinite(want).all()
    differ = np.nonzero(bits(got) != bits(want))[0]
    print('%d pairs, %d runs: %d scores differ in their bits' % (prob.n, len(prob.runs()), differ.size))
    assert differ.size == 0, (differ[:8], got[differ[:8]], want[differ[:8]])
    assert_fence_intact(be, scores, 'scores')
    assert_fence_intact(be, dev.desc, 'descriptors')
    return dev, got


_PROBLEMS = {}


def problem(*args, **kwargs):
    key = (args, tuple(sorted(kwargs.items())))
    if key not in _PROBLEMS:
        _PROBLEMS[key] = Problem(*args, **kwargs)
    return _PROBLEMS[key]


@pytest.mark.parametrize('D', [16, 48])
@pytest.mark.parametrize('qt', TYPES)
def test_every_type_three_formulas(be, qt, D):
    prob = problem(qt, D, 3, RUNS_MAIN, 100 * TYPES.index(qt) + D)
    assert len(set(prob.formulas)) == 3 and len({tuple(p) for p in prob.progs}) == 3
    assert sorted(set(prob.neg_lengths)) == sorted(NEG_COUNTS) and prob.B == 34
    check(be, prob)


def test_largest_dim(be):
    prob = problem('3-inter_chain', 256, 3, ((0, 1), (1, 2), (2, 2)), 5, neg_counts=(0, 1, 17))
    check(be, prob)


@pytest.mark.parametrize('qt', ['2-chain', '3-inter'])
def test_every_query_a_formula_of_its_own(be, qt):
    prob = problem(qt, 48, 33, tuple((f, 1) for f in range(33)), 11, neg_counts=(0, 1, 17))
    assert prob.B == prob.F == 33
    check(be, prob)


@pytest.mark.parametrize('qt', ['3-chain', '3-chain_inter'])
def test_unused_and_returning_formulas(be, qt):
    """formula 1 is listed and never used; formula 0 returns in a second run that is not adjacent to its first"""
    prob = problem(qt, 48, 4, ((0, 3), (2, 17), (0, 2), (3, 1)), 21)
    assert 1 not in prob.formula_of and len(prob.runs()) == 4
    check(be, prob)


@pytest.mark.parametrize('qt', ['1-chain', '2-inter'])
def test_no_queries(be, qt):
    prob = problem(qt, 48, 2, (), 31)
    assert prob.B == 0 and prob.n == 0
    dev = Device(be, prob)
    assert dev.build() == OK
    st, scores = dev.mixed()
    assert st == OK and int(be.get(dev.err)[0]) == 0
    assert_fence_intact(be, dev.desc, 'descriptors')


@pytest.mark.parametrize('qt', ['2-chain', '3-inter_chain', '3-chain_inter'])
@pytest.mark.parametrize('op', ['translate', 'scale'])
def test_vector_operators(be, qt, op):
    prob = problem(qt, 48, 3, RUNS_MAIN, 41 + TYPES.index(qt), op=op)
    assert prob.progs[0][7] == {'translate': 1, 'scale': 2}[op]
    check(be, prob)


@pytest.mark.parametrize('qt', ['1-chain', '3-chain'])
def test_dot_scoring_on_diagonal_chains(be, qt):
    prob = problem(qt, 48, 3, RUNS_MAIN, 51, op='scale', score='dot')
    assert prob.progs[0][27] == 1
    check(be, prob)


@pytest.mark.parametrize('qt', ['2-inter', '3-inter', '3-inter_chain', '3-chain_inter'])
@pytest.mark.parametrize('inter', ['min', 'mean-simple', 'min-simple'])
def test_aggregates_with_and_without_pre_post(be, qt, inter):
    prob = problem(qt, 48, 3, RUNS_MAIN, 61 + TYPES.index(qt), inter=inter)
    assert prob.progs[0][2] == int(inter.startswith('min')) and (prob.progs[0][3] < 0) == inter.endswith('simple')
    check(be, prob)


@pytest.mark.parametrize('qt', ['2-chain', '2-inter'])
def test_one_relation_at_two_sites(be, qt):
    prob = problem(qt, 48, 2, ((0, 5), (1, 17), (0, 1)), 71, repeat=True)
    assert all(f.rels[0] == f.rels[1] for f in prob.formulas)
    check(be, prob)


@pytest.mark.parametrize('qt', ['2-chain', '3-inter'])
def test_bad_id_flags_and_spares_the_other_queries(be, qt):
    prob = problem(qt, 48, 3, RUNS_MAIN, 100 * TYPES.index(qt) + 48)
    dev, want = check(be, prob)
    victim = 20
    anchors = prob.anchors.copy()
    anchors[victim, 0] = prob.params.node_map.shape[0] - 1          # (in the map, of no mode: -1)
    st, scores = dev.mixed(anchors=anchors)
    assert st == OK and int(be.get(dev.err)[0]) == FLAG_BAD_NODE_ID
    got = be.get(scores)
    q_of = np.concatenate([np.arange(prob.B), np.repeat(np.arange(prob.B), prob.neg_lengths)])
    assert np.isfinite(got).all()
    np.testing.assert_array_equal(bits(got[q_of != victim]), bits(want[q_of != victim]))
    assert (bits(got[q_of == victim]) != bits(want[q_of == victim])).any()
    assert_fence_intact(be, scores, 'scores')


@pytest.mark.parametrize('bad', [-1, 3, 2 ** 40])
@pytest.mark.parametrize('qt', ['2-chain', '3-inter'])
def test_bad_formula_index_flags_and_spares_the_other_queries(be, qt, bad):
    prob = problem(qt, 48, 3, RUNS_MAIN, 100 * TYPES.index(qt) + 48)
    dev, want = check(be, prob)
    victim = 21                                    # (inside the run of 17: it is cut in two)
    fo = prob.formula_of.copy()
    fo[victim] = bad
    st, scores = dev.mixed(formula_of=fo)
    assert st == OK and int(be.get(dev.err)[0]) == FLAG_BAD_INDEX
    got = be.get(scores)
    q_of = np.concatenate([np.arange(prob.B), np.repeat(np.arange(prob.B), prob.neg_lengths)])
    np.testing.assert_array_equal(bits(got[q_of != victim]), bits(want[q_of != victim]))
    assert (got[q_of == victim] == 0).all()
    assert_fence_intact(be, scores, 'scores')


def test_programmes_that_disagree_are_refused(be):
    """another form, another operator, another branch count: MPQE_ERR_INVALID_ARG before anything is written"""
    prob = problem('2-inter', 48, 3, RUNS_MAIN, 100 * TYPES.index('2-inter') + 48)
    others = [problem('2-chain', 48, 3, RUNS_MAIN, 100 * TYPES.index('2-chain') + 48).progs[1],
              problem('3-inter', 48, 3, RUNS_MAIN, 100 * TYPES.index('3-inter') + 48).progs[1]]
    op = prob.progs[1].copy()
    op[7] = 2
    agg = prob.progs[1].copy()
    agg[2] = 1
    dev = Device(be, prob)
    for other in others + [op, agg]:
        progs = prob.progs.copy()
        progs[2] = other
        assert dev.build(fill='noise', progs=progs) == INVALID
        image = np.resize(FILLS['noise'], dev.desc_bytes)
        np.testing.assert_array_equal(be.get(dev.desc), image)
        assert_fence_intact(be, dev.desc, 'descriptors')


@pytest.mark.parametrize('fill', ['zeros', 'nan', 'ones', 'noise'])
def test_descriptor_block_is_exactly_its_declared_size(be, fill):
    prob = problem('3-inter', 48, 3, RUNS_MAIN, 100 * TYPES.index('3-inter') + 48)
    dev = Device(be, prob)
    want = dev.per_formula()
    assert dev.build(fill=fill) == OK
    st, scores = dev.mixed()
    assert st == OK
    np.testing.assert_array_equal(bits(be.get(scores)), bits(want))
    assert_fence_intact(be, dev.desc, 'descriptors')
    # one byte short: refused by the build and by the scoring call, nothing written
    assert dev.build(fill=fill, short=1) == WORKSPACE
    before = be.get(dev.desc).copy()
    assert_fence_intact(be, dev.desc, 'descriptors')
    st, scores = dev.mixed(short=1)
    assert st == WORKSPACE
    np.testing.assert_array_equal(be.get(dev.desc), before)
    assert (be.get(scores) == np.float32(7.5)).all()
    assert be.lib.mpqe_gqe_mixed_desc_bytes(0) == 0


def test_run_to_run_bits(be):
    prob = problem('3-inter_chain', 48, 3, RUNS_MAIN, 100 * TYPES.index('3-inter_chain') + 48)
    dev = Device(be, prob)
    assert dev.build() == OK
    runs = []
    for _ in range(2):
        st, scores = dev.mixed()
        assert st == OK
        runs.append(be.get(scores).tobytes())
    assert runs[0] == runs[1]
