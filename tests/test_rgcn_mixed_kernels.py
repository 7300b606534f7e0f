"""mpqe_rgcn_fwd_mixed / mpqe_rgcn_embed_mixed / mpqe_rgcn_mixed_desc_build (csrc/rgcn_mixed.hip) through the C ABI, on the
host emulator and on the GPU (the `be` fixture of tests/test_gqe_kernels.py): R-GCN queries of DIFFERENT formulas of one
query type encoded in one launch and scored in a second.

The oracle is the module path's entry points on the same backend, handed every run of equal formula alone:
mpqe_embed_l2norm_fwd per anchor slot + mpqe_var_rows_fwd -> mpqe_rgcn_template_fwd per pass -> mpqe_readout_fwd ->
mpqe_embed_l2norm_fwd + mpqe_cosine_fwd. Scores and query embeddings are compared as uint32 BITS (the contract of
include/mpqe_amd.h: no tolerance). Every operand sits between fences (tests/fenced.py): a read outside an id list meets the
integer fence (no id, no formula: the error word is set, which every clean case asserts it is not), a read outside a
table or a matrix meets a NaN, a write outside the scores, the descriptor block or the workspace is caught bit for bit.

Shapes: D 16 (one partial K-step, a partial column tile) / 48 (two K-steps, the second partial) / 128 (two column tiles,
four K-steps); all seven query types; run lengths 1, 63, 64, 65, 1, 1 (stretches that end one short of, at and one past a
64-query block, several stretches in one block); negative counts 0, 1, 63, 64, 65, 300 per query."""
import ctypes

import numpy as np
import pytest

from mpqe_amd import _capi
from tests.fenced import FILLS, assert_fence_intact, fenced, fenced_bytes
from tests.test_gqe_kernels import INVALID, OK, TYPES, UNSUPPORTED, WORKSPACE, be  # noqa: F401  (`be`: the backend fixture)

ROWS, MODES, RELS = 23, 3, 5
NEG_COUNTS = (0, 1, 63, 64, 65, 300)
NEG_FEW = (0, 1, 65)            # the tests that are not about the negatives
RUNS_MAIN = ((0, 1), (1, 63), (2, 64), (3, 65), (4, 1), (5, 1))          # (formula, run length)
FLAG_BAD_NODE_ID, FLAG_BAD_RELATION, FLAG_BAD_INDEX = 1, 4, 8
READOUTS = _capi.READOUT_IDS
REC = _capi.RGCN_MIX_REC_INTS


def template(qt):
    from mpqe_amd import _lib
    info = _capi.TemplateInfo()
    assert _lib.load().mpqe_template_info(_capi.QUERY_TYPE_IDS[qt], info) == 0
    return info


class Problem(object):
    """Q queries of one query type under F formulas over one set of tables, mode embeddings and layers. layers: how many
    distinct layers there are -- pass p runs layer p, the last pass the LAST layer (RGCNEncoderDecoder.encode); 1 = shared."""

    def __init__(self, qt, D, F, runs, seed, passes=None, readout='mp', layers=3, bias=True, neg_counts=NEG_COUNTS,
                 repeat=False, same_target=False, duplicate_anchors=False):
        rng = np.random.RandomState(seed)
        info = template(qt)
        self.qt, self.qid, self.D, self.F = qt, _capi.QUERY_TYPE_IDS[qt], D, F
        self.A, self.V, self.N, self.E = info.num_anchors, info.num_vars, info.num_nodes, info.num_edges
        self.passes = info.diameter if passes is None else passes
        self.readout = readout
        n_ent = ROWS * MODES
        self.node_map = np.full(n_ent + 1, -1, dtype=np.int64)
        self.ids = []
        for m in range(MODES):
            self.ids.append(np.arange(m, n_ent, MODES, dtype=np.int64))
            self.node_map[self.ids[m]] = np.arange(ROWS)
        self.tables = [rng.normal(0, 1.0, (ROWS + m, D)).astype(np.float32) for m in range(MODES)]
        self.mode_emb = rng.normal(0, 1.0, (MODES, D)).astype(np.float32)
        bound = 3.0 / np.sqrt(RELS * D)
        self.layers = [(rng.uniform(-bound, bound, (RELS, D, D)).astype(np.float32),
                        rng.uniform(-bound, bound, (D, D)).astype(np.float32),
                        rng.uniform(-bound, bound, (D,)).astype(np.float32) if bias else None) for _ in range(layers)]
        self.layer_of_pass = [min(p, layers - 1) for p in range(self.passes - 1)] + [layers - 1]
        self.recs = np.zeros((F, REC), dtype=np.int32)
        for f in range(F):
            while True:
                rec = np.zeros(REC, dtype=np.int32)
                rec[0:self.E] = rng.randint(0, RELS, self.E)
                rec[3:3 + self.A] = rng.randint(0, MODES, self.A)
                rec[6:6 + self.V] = rng.randint(0, MODES, self.V)
                rec[9] = 0 if same_target else rng.randint(0, MODES)
                if repeat:        # anchor slots that share a table, variable slots that repeat a mode row
                    rec[3:3 + self.A] = rec[3]
                    rec[6:6 + self.V] = rec[6]
                if F > 40 or not any((rec == r).all() for r in self.recs[:f]):
                    break
            self.recs[f] = rec
        self.formula_of = np.concatenate([np.full(k, f, dtype=np.int64) for f, k in runs] + [np.zeros(0, dtype=np.int64)])
        Q = self.Q = int(self.formula_of.shape[0])
        self.anchors = np.zeros((Q, self.A), dtype=np.int64)
        self.targets = np.zeros(Q, dtype=np.int64)
        self.neg_lengths = np.array([neg_counts[q % len(neg_counts)] for q in range(Q)], dtype=np.int64)
        negs = []
        for q in range(Q):
            rec = self.recs[self.formula_of[q]]
            self.anchors[q] = [rng.choice(self.ids[rec[3 + a]]) for a in range(self.A)]
            if duplicate_anchors and q % 2 == 0:
                self.anchors[q] = self.anchors[q, 0]
            self.targets[q] = rng.choice(self.ids[rec[9]])
            negs.append(rng.choice(self.ids[rec[9]], size=int(self.neg_lengths[q])))
        self.negs = np.concatenate(negs + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
        self.neg_off = np.concatenate([[0], np.cumsum(self.neg_lengths)]).astype(np.int64)
        self.pair_ids = np.concatenate([self.targets, self.negs]).astype(np.int64)
        self.qrow = np.concatenate([np.arange(Q), np.repeat(np.arange(Q), self.neg_lengths)]).astype(np.int64)
        self.n = int(self.pair_ids.shape[0])

    def runs(self):
        from mpqe_amd.model import formula_runs
        return formula_runs(self.formula_of)


def place(be, a):
    """fenced(); an empty operand (whose view would forget its address) is a plain empty array"""
    a = np.asarray(a)
    return fenced(be, a) if a.size else be.put(a)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Device(object):
    """A problem's shared operands on a backend, fenced, the module path run by run and the mixed calls."""

    def __init__(self, be, prob):
        self.be, self.prob = be, prob
        self.tables = [fenced(be, t) for t in prob.tables]
        self.mode_emb = fenced(be, prob.mode_emb)
        self.node_map = fenced(be, prob.node_map)
        self.layers = [(fenced(be, b), fenced(be, r), None if bi is None else fenced(be, bi)) for b, r, bi in prob.layers]
        self.tab = (ctypes.c_void_p * MODES)(*[be.ptr(t) for t in self.tables])
        self.rows = (ctypes.c_int64 * MODES)(*[int(t.shape[0]) for t in self.tables])
        self.err = be.zeros(1, np.int32)
        self.set_passes(prob.passes, prob.layer_of_pass)

    def set_passes(self, passes, layer_of_pass, no_bias_array=False):
        self.passes = passes
        n = max(passes, 1)
        pick = [self.layers[l] for l in layer_of_pass] + [self.layers[-1]] * (n - len(layer_of_pass))
        self.basis = (ctypes.c_void_p * n)(*[self.be.ptr(l[0]) for l in pick[:n]])
        self.root = (ctypes.c_void_p * n)(*[self.be.ptr(l[1]) for l in pick[:n]])
        self.bias = None if no_bias_array else (ctypes.c_void_p * n)(*[self.be.ptr(l[2]) for l in pick[:n]])
        self.picked = pick[:n]

    def module_path(self, anchors=None, pair_ids=None):
        """the oracle: every run through the per-op entry points -> (scores in the layout of the whole, q_out [Q, D])"""
        be, prob, lib = self.be, self.prob, self.be.lib
        D, N, A, V = prob.D, prob.N, prob.A, prob.V
        anchors = prob.anchors if anchors is None else anchors
        pair_ids = prob.pair_ids if pair_ids is None else pair_ids
        scores, q_all = np.zeros(prob.n, dtype=np.float32), np.zeros((prob.Q, D), dtype=np.float32)
        nm, nm_len = be.ptr(self.node_map), int(self.node_map.shape[0])
        for f, lo, hi in prob.runs():
            rec, B = prob.recs[f], hi - lo
            x = be.empty((B * N, D))
            keep = []
            for a in range(A):
                ids = be.put(np.ascontiguousarray(anchors[lo:hi, a]))
                keep.append(ids)
                t = self.tables[rec[3 + a]]
                assert lib.mpqe_embed_l2norm_fwd(be.ptr(t), int(t.shape[0]), D, nm, nm_len, be.ptr(ids), B,
                                                 be.ptr(x) + 4 * a * D, N * D, None, be.ptr(self.err), be.stream) == OK
            var = be.put(rec[6:6 + V].astype(np.int64))
            assert lib.mpqe_var_rows_fwd(be.ptr(self.mode_emb), MODES, D, be.ptr(var), V, B, N, A, be.ptr(x), be.ptr(self.err),
                                         be.stream) == OK
            et = np.ascontiguousarray(rec[0:prob.E].astype(np.int64))
            h = x
            for p in range(self.passes):
                basis, root, bias = self.picked[p]
                out = be.empty((B * N, D))
                assert lib.mpqe_rgcn_template_fwd(prob.qid, B, et.ctypes.data, be.ptr(h), be.ptr(basis), RELS, be.ptr(root),
                                                  be.ptr(bias), D, D, int(p < self.passes - 1), be.ptr(out), be.stream) == OK
                h = out
            q = be.empty((B, D))
            assert lib.mpqe_readout_fwd(READOUTS[prob.readout], be.ptr(h), B, N, A, D, be.ptr(q), None, be.stream) == OK
            a0, b0 = int(prob.neg_off[lo]), int(prob.neg_off[hi])
            ids = np.concatenate([pair_ids[lo:hi], pair_ids[prob.Q + a0:prob.Q + b0]]).astype(np.int64)
            qrow = np.concatenate([np.arange(B), np.repeat(np.arange(B), prob.neg_lengths[lo:hi])]).astype(np.int64)
            ids_d, qrow_d = be.put(ids), be.put(qrow)
            n_run = int(ids.shape[0])
            tt = self.tables[rec[9]]
            t = be.empty((n_run, D))
            assert lib.mpqe_embed_l2norm_fwd(be.ptr(tt), int(tt.shape[0]), D, nm, nm_len, be.ptr(ids_d), n_run, be.ptr(t), D,
                                             None, be.ptr(self.err), be.stream) == OK
            s = be.empty((n_run,))
            assert lib.mpqe_cosine_fwd(be.ptr(q), be.ptr(qrow_d), be.ptr(t), n_run, D, 1e-8, be.ptr(s), be.stream) == OK
            got = be.get(s)
            scores[lo:hi] = got[:B]
            scores[prob.Q + a0:prob.Q + b0] = got[B:]
            q_all[lo:hi] = be.get(q)
        return scores, q_all

    def build(self, fill='nan', short=0, recs=None, mode_rows=MODES, qid=None):
        be, prob = self.be, self.prob
        recs = np.ascontiguousarray(prob.recs if recs is None else recs, dtype=np.int32)
        self.desc_bytes = be.lib.mpqe_rgcn_mixed_desc_bytes(recs.shape[0])
        assert self.desc_bytes > 0 and self.desc_bytes % 256 == 0
        self.desc = fenced_bytes(be, self.desc_bytes - short, fill)
        return be.lib.mpqe_rgcn_mixed_desc_build(prob.qid if qid is None else qid, recs.ctypes.data, recs.shape[0], self.tab,
                                                 self.rows, MODES, mode_rows, be.ptr(self.desc), self.desc_bytes - short,
                                                 be.stream)

    def workspace(self, fill='nan', short=0, misalign=0):
        prob = self.prob
        self.ws_bytes = self.be.lib.mpqe_rgcn_mixed_workspace_bytes(prob.qid, prob.Q, prob.D)
        self.ws = fenced_bytes(self.be, self.ws_bytes - short, fill, misalign=misalign)

    def mixed(self, formula_of=None, anchors=None, pair_ids=None, qrow=None, short=0, ws_short=0, embed=False, **over):
        """-> (status, scores view) of mpqe_rgcn_fwd_mixed, or (status, q_out view) of mpqe_rgcn_embed_mixed"""
        be, prob = self.be, self.prob
        if not hasattr(self, 'ws'):
            self.workspace()
        a = dict(qid=prob.qid, F=prob.F, desc=be.ptr(self.desc), node_map=be.ptr(self.node_map),
                 mode_emb=be.ptr(self.mode_emb), basis=self.basis, root=self.root, bias=self.bias, R=RELS,
                 passes=self.passes, readout=READOUTS[prob.readout], D=prob.D, Q=prob.Q, ws=be.ptr(self.ws))
        fo = place(be, prob.formula_of if formula_of is None else formula_of)
        an = place(be, prob.anchors if anchors is None else anchors)
        ids = place(be, prob.pair_ids if pair_ids is None else pair_ids)
        qr = place(be, prob.qrow if qrow is None else qrow)
        a.update(fo_ptr=be.ptr(fo), an_ptr=be.ptr(an), ids_ptr=be.ptr(ids), qrow_ptr=be.ptr(qr))
        a.update(over)
        self.keep = [fo, an, ids, qr]
        head = (a['qid'], a['F'], a['desc'], self.desc_bytes - short, a['node_map'], int(self.node_map.shape[0]), a['mode_emb'],
                a['basis'], a['root'], a['bias'], a['R'], a['passes'], a['readout'], a['D'], a['fo_ptr'], a['an_ptr'], a['Q'])
        if embed:
            out = place(be, np.full((prob.Q, prob.D), np.float32(7.5)))
            st = be.lib.mpqe_rgcn_embed_mixed(*head, a['ws'], self.ws_bytes - ws_short, be.ptr(out), be.ptr(self.err), be.stream)
            return st, out
        scores = place(be, np.full(prob.n, np.float32(7.5)))
        st = be.lib.mpqe_rgcn_fwd_mixed(*head, a['ids_ptr'], a['qrow_ptr'], prob.n, 1e-8, a['ws'], self.ws_bytes - ws_short,
                                        be.ptr(scores), be.ptr(self.err), be.stream)
        return st, scores


_PROBLEMS, _ORACLES = {}, {}


def problem(*args, **kwargs):
    key = (args, tuple(sorted(kwargs.items())))
    if key not in _PROBLEMS:
        _PROBLEMS[key] = Problem(*args, **kwargs)
        _PROBLEMS[key].key = key
    return _PROBLEMS[key]


def oracle(be, dev):
    """the module path's scores and embeddings of a problem on a backend: computed once, shared, left unchanged"""
    key = (be.name, dev.prob.key, dev.passes, tuple(id(l) for l in dev.picked), dev.bias is None)
    if key not in _ORACLES:
        _ORACLES[key] = dev.module_path()
        assert int(be.get(dev.err)[0]) == 0
    return _ORACLES[key]


def check(be, prob, dev=None):
    dev = Device(be, prob) if dev is None else dev
    want, want_q = oracle(be, dev)
    assert dev.build() == OK
    st, scores = dev.mixed()
    assert st == OK
    got = be.get(scores)
    assert int(be.get(dev.err)[0]) == 0
    assert np.isfinite(want).all() and np.abs(want).max() <= 1.0 + 1e-5 and want.std() > 0 if prob.n > 1 else True
    differ = np.nonzero(bits(got) != bits(want))[0]
    print('%d pairs, %d runs: %d scores differ in their bits' % (prob.n, len(prob.runs()), differ.size))
    assert differ.size == 0, (differ[:8], got[differ[:8]], want[differ[:8]])
    assert_fence_intact(be, scores, 'scores')
    assert_fence_intact(be, dev.desc, 'descriptors')
    assert_fence_intact(be, dev.ws, 'workspace')
    return dev, got


def test_symbols_are_declared_and_exported(be):
    for name in ('mpqe_rgcn_mixed_desc_bytes', 'mpqe_rgcn_mixed_desc_build', 'mpqe_rgcn_mixed_workspace_bytes',
                 'mpqe_rgcn_embed_mixed', 'mpqe_rgcn_fwd_mixed'):
        assert name in _capi.PROTOTYPES and hasattr(be.lib, name)
    assert be.lib.mpqe_abi_version() == 7
    assert be.lib.mpqe_rgcn_mixed_desc_bytes(0) == 0 and be.lib.mpqe_rgcn_mixed_desc_bytes(1) == 256
    assert be.lib.mpqe_rgcn_mixed_workspace_bytes(7, 4, 16) == 0 and be.lib.mpqe_rgcn_mixed_workspace_bytes(0, -1, 16) == 0
    # two state buffers [Q * N, D] and the embeddings [Q, D], each rounded up to 256 bytes
    assert be.lib.mpqe_rgcn_mixed_workspace_bytes(2, 5, 48) == 2 * 3840 + 1024


@pytest.mark.parametrize('D', [16, 48, 128])
@pytest.mark.parametrize('qt', TYPES)
def test_every_type_six_formulas(be, qt, D):
    prob = problem(qt, D, 6, RUNS_MAIN, 100 * TYPES.index(qt) + D)
    assert len({tuple(r) for r in prob.recs}) == 6 and prob.Q == 195
    assert sorted(set(prob.neg_lengths)) == sorted(NEG_COUNTS)
    dev, _ = check(be, prob)
    # the encode launch alone writes the module path's query embeddings
    st, q_out = dev.mixed(embed=True)
    assert st == OK
    np.testing.assert_array_equal(bits(be.get(q_out)), bits(oracle(be, dev)[1]))
    assert_fence_intact(be, q_out, 'q_out')


@pytest.mark.parametrize('qt', ['2-chain', '3-inter'])
def test_every_query_a_formula_of_its_own(be, qt):
    prob = problem(qt, 48, 70, tuple((f, 1) for f in range(70)), 11, neg_counts=NEG_FEW)
    assert prob.Q == prob.F == 70
    check(be, prob)


@pytest.mark.parametrize('qt', ['3-chain', '3-chain_inter'])
def test_one_formula_throughout(be, qt):
    prob = problem(qt, 48, 2, ((1, 130),), 13, neg_counts=NEG_FEW)
    assert len(prob.runs()) == 1
    check(be, prob)


@pytest.mark.parametrize('qt', ['1-chain', '3-inter_chain'])
def test_without_negatives(be, qt):
    """neg = None: n == num_queries, qrow the identity"""
    prob = problem(qt, 48, 6, RUNS_MAIN, 17, neg_counts=(0,))
    assert prob.n == prob.Q
    check(be, prob)


@pytest.mark.parametrize('layers', [1, 3])
@pytest.mark.parametrize('passes', [1, 2, 3])
def test_passes_and_the_last_layer_rule(be, passes, layers):
    """pass p < passes - 1 runs layer p with ReLU, the last pass the LAST layer without (encode()'s self.layers[-1])"""
    prob = problem('3-inter_chain', 48, 3, ((0, 5), (1, 66), (2, 3)), 23, passes=passes, layers=layers, neg_counts=NEG_FEW)
    assert prob.layer_of_pass == ([0, 1][:passes - 1] + [2] if layers == 3 else [0] * passes)
    check(be, prob)


@pytest.mark.parametrize('how', ['no_bias', 'no_bias_array'])
def test_bias_absent(be, how):
    prob = problem('2-inter', 48, 3, ((0, 5), (1, 66), (2, 3)), 29, bias=how != 'no_bias', neg_counts=NEG_FEW)
    dev = Device(be, prob)
    if how == 'no_bias_array':
        # (the oracle then runs without the bias too)
        dev.layers = [(b, r, None) for b, r, _ in dev.layers]
        dev.set_passes(prob.passes, prob.layer_of_pass, no_bias_array=True)
    assert all(l[2] is None for l in dev.picked)
    check(be, prob, dev)


@pytest.mark.parametrize('readout', ['sum', 'max'])
@pytest.mark.parametrize('qt', ['2-chain', '2-inter', '3-inter'])
def test_sum_and_max_readouts(be, qt, readout):
    """every other query's anchors are ONE entity of one table: equal node states, a tie under max"""
    prob = problem(qt, 48, 4, ((0, 5), (1, 66), (2, 3), (3, 2)), 31 + TYPES.index(qt), readout=readout, repeat=True,
                   duplicate_anchors=True, neg_counts=NEG_FEW)
    if prob.A > 1:
        assert (prob.anchors[0] == prob.anchors[0, 0]).all()
    check(be, prob)


@pytest.mark.parametrize('qt', ['3-chain', '3-inter', '3-chain_inter'])
def test_repeated_modes(be, qt):
    """anchor slots that share a table, variable slots that repeat a mode row"""
    prob = problem(qt, 16, 3, ((0, 5), (1, 66), (2, 3)), 37, repeat=True, neg_counts=NEG_FEW)
    assert all(len(set(r[3:3 + prob.A])) == 1 and len(set(r[6:6 + prob.V])) == 1 for r in prob.recs)
    check(be, prob)


def q_of(prob):
    return prob.qrow


@pytest.mark.parametrize('bad', [-1, 6, 2 ** 40])
@pytest.mark.parametrize('qt', ['2-chain', '3-inter'])
def test_bad_formula_index_flags_and_spares_the_other_queries(be, qt, bad):
    prob = problem(qt, 48, 6, RUNS_MAIN, 100 * TYPES.index(qt) + 48, neg_counts=NEG_FEW)
    dev, want = check(be, prob)
    victim = 70                                    # (inside the run of 64: it is cut in two)
    fo = prob.formula_of.copy()
    fo[victim] = bad
    st, scores = dev.mixed(formula_of=fo)
    assert st == OK and int(be.get(dev.err)[0]) == FLAG_BAD_INDEX
    got = be.get(scores)
    np.testing.assert_array_equal(bits(got[q_of(prob) != victim]), bits(want[q_of(prob) != victim]))
    assert (bits(got[q_of(prob) == victim]) == 0).all() and (q_of(prob) == victim).sum() > 1
    assert_fence_intact(be, scores, 'scores')
    assert_fence_intact(be, dev.ws, 'workspace')


@pytest.mark.parametrize('bad', [-1, 195, 2 ** 40])
def test_bad_qrow_flags_and_scores_zero(be, bad):
    prob = problem('3-inter', 48, 6, RUNS_MAIN, 100 * TYPES.index('3-inter') + 48, neg_counts=NEG_FEW)
    dev, want = check(be, prob)
    rows = np.array([3, prob.Q + 7, prob.n - 1])
    qrow = prob.qrow.copy()
    qrow[rows] = bad
    st, scores = dev.mixed(qrow=qrow)
    assert st == OK and int(be.get(dev.err)[0]) == FLAG_BAD_INDEX
    got = be.get(scores)
    keep = np.ones(prob.n, dtype=bool)
    keep[rows] = False
    np.testing.assert_array_equal(bits(got[keep]), bits(want[keep]))
    assert (bits(got[rows]) == 0).all()
    assert_fence_intact(be, scores, 'scores')


@pytest.mark.parametrize('qt', ['2-chain', '3-inter'])
def test_bad_ids_flag_and_keep_the_module_paths_bits(be, qt):
    """a bad anchor id and a bad target id: the looked-up row is zeros on both paths"""
    prob = problem(qt, 48, 6, RUNS_MAIN, 100 * TYPES.index(qt) + 48, neg_counts=NEG_FEW)
    dev, clean = check(be, prob)
    no_mode = prob.node_map.shape[0] - 1          # (in the map, of no mode: -1)
    anchors, pair_ids = prob.anchors.copy(), prob.pair_ids.copy()
    anchors[70, 0] = no_mode
    anchors[3, prob.A - 1] = 10 ** 12
    pair_ids[5] = no_mode
    pair_ids[prob.Q + 9] = -4
    st, scores = dev.mixed(anchors=anchors, pair_ids=pair_ids)
    assert st == OK and int(be.get(dev.err)[0]) == FLAG_BAD_NODE_ID
    got = be.get(scores)
    dev.err[...] = 0
    want, _ = dev.module_path(anchors=anchors, pair_ids=pair_ids)
    assert int(be.get(dev.err)[0]) == FLAG_BAD_NODE_ID
    np.testing.assert_array_equal(bits(got), bits(want))
    touched = np.isin(prob.qrow, [70, 3])
    touched[[5, prob.Q + 9]] = True
    np.testing.assert_array_equal(bits(got[~touched]), bits(clean[~touched]))
    assert (bits(got[touched]) != bits(clean[touched])).any()
    assert_fence_intact(be, scores, 'scores')


def test_relation_outside_the_call_s_count_flags(be):
    """the descriptor block does not know num_relations: a relation past it is caught in the launch, nothing is read"""
    prob = problem('2-chain', 48, 6, RUNS_MAIN, 100 * TYPES.index('2-chain') + 48, neg_counts=NEG_FEW)
    dev, want = check(be, prob)
    low = int(prob.recs[:, 0:prob.E].max())
    assert low > 0
    st, scores = dev.mixed(R=low)
    got = be.get(scores)
    hit = np.array([(prob.recs[k, 0:prob.E] >= low).any() for k in range(prob.F)])[prob.formula_of[prob.qrow]]
    assert st == OK and int(be.get(dev.err)[0]) == FLAG_BAD_RELATION and hit.any() and not hit.all()
    assert (bits(got[hit]) == 0).all()
    np.testing.assert_array_equal(bits(got[~hit]), bits(want[~hit]))
    assert_fence_intact(be, scores, 'scores')


def test_descriptor_build_checks_every_field(be):
    prob = problem('3-inter_chain', 48, 3, ((0, 5), (1, 66), (2, 3)), 41, neg_counts=NEG_FEW)
    dev = Device(be, prob)
    cases = [(0, -1), (prob.E - 1, -2), (3, MODES), (3 + prob.A - 1, -1), (6, MODES), (6 + prob.V - 1, -1), (9, MODES), (9, -1)]
    for col, value in cases:
        recs = prob.recs.copy()
        recs[2, col] = value
        assert dev.build(fill='noise', recs=recs) == INVALID, (col, value)
        np.testing.assert_array_equal(be.get(dev.desc), np.resize(FILLS['noise'], dev.desc_bytes))
        assert_fence_intact(be, dev.desc, 'descriptors')
    assert dev.build(qid=7) == INVALID and dev.build(mode_rows=0) == INVALID
    # a mode-embedding row past the rows the build was told of
    assert dev.build(mode_rows=int(prob.recs[:, 6:6 + prob.V].max())) == INVALID
    # entries past the template's edges / anchors / variables are not read
    recs = prob.recs.copy()
    recs[:, 3 + prob.A:6] = -9
    recs[:, 6 + prob.V:9] = -9
    assert dev.build(recs=recs) == OK


@pytest.mark.parametrize('fill', sorted(FILLS))
def test_descriptor_block_and_workspace_are_exactly_their_declared_size(be, fill):
    prob = problem('3-inter', 48, 6, RUNS_MAIN, 100 * TYPES.index('3-inter') + 48, neg_counts=NEG_FEW)
    dev = Device(be, prob)
    want, _ = oracle(be, dev)
    assert dev.build(fill=fill) == OK
    dev.workspace(fill=fill)
    st, scores = dev.mixed()
    assert st == OK
    np.testing.assert_array_equal(bits(be.get(scores)), bits(want))
    assert_fence_intact(be, dev.desc, 'descriptors')
    assert_fence_intact(be, dev.ws, 'workspace')
    # one byte short: refused, nothing written
    dev.workspace(fill=fill, short=1)
    before = be.get(dev.ws).copy()
    for embed in (False, True):
        st, out = dev.mixed(ws_short=1, embed=embed)
        assert st == WORKSPACE
        assert (be.get(out) == np.float32(7.5)).all()
        np.testing.assert_array_equal(be.get(dev.ws), before)
        assert_fence_intact(be, dev.ws, 'workspace')
    assert dev.build(fill=fill, short=1) == WORKSPACE
    np.testing.assert_array_equal(be.get(dev.desc), np.resize(FILLS[fill], dev.desc_bytes - 1))
    assert_fence_intact(be, dev.desc, 'descriptors')
    dev.workspace(fill=fill)
    st, out = dev.mixed(short=1)
    assert st == WORKSPACE and (be.get(out) == np.float32(7.5)).all()
    assert int(be.get(dev.err)[0]) == 0


def test_refusals_come_before_any_launch(be):
    prob = problem('3-inter', 48, 6, RUNS_MAIN, 100 * TYPES.index('3-inter') + 48, neg_counts=NEG_FEW)
    dev = Device(be, prob)
    assert dev.build() == OK
    dev.workspace(fill='noise')
    image = be.get(dev.ws).copy()
    shifted = (ctypes.c_void_p * dev.passes)(*[be.ptr(l[0]) + 4 for l in dev.picked])
    nulls = (ctypes.c_void_p * dev.passes)(*[None] * dev.passes)
    cases = [(UNSUPPORTED, dict(D=18)), (UNSUPPORTED, dict(D=0 + 50)), (UNSUPPORTED, dict(passes=0)), (UNSUPPORTED, dict(passes=5)),
             (UNSUPPORTED, dict(readout=3)), (UNSUPPORTED, dict(readout=4)), (UNSUPPORTED, dict(ws=be.ptr(dev.ws) + 4)),
             (UNSUPPORTED, dict(basis=shifted)), (UNSUPPORTED, dict(root=shifted)), (UNSUPPORTED, dict(mode_emb=be.ptr(dev.mode_emb) + 4)),
             (INVALID, dict(qid=7)), (INVALID, dict(qid=-1)), (INVALID, dict(F=0)), (INVALID, dict(desc=None)),
             (INVALID, dict(desc=be.ptr(dev.desc) + 16)), (INVALID, dict(fo_ptr=None)), (INVALID, dict(an_ptr=None)),
             (INVALID, dict(mode_emb=None)), (INVALID, dict(ws=None)), (INVALID, dict(basis=None)), (INVALID, dict(root=nulls)),
             (INVALID, dict(R=0)), (INVALID, dict(D=-4)), (INVALID, dict(Q=-1))]
    for embed in (False, True):
        more = [] if embed else [(INVALID, dict(ids_ptr=None)), (INVALID, dict(qrow_ptr=None))]
        for status, over in cases + more:
            st, out = dev.mixed(embed=embed, **over)
            assert st == status, (embed, over, st)
            assert (be.get(out) == np.float32(7.5)).all(), over
            np.testing.assert_array_equal(be.get(dev.ws), image)
    assert int(be.get(dev.err)[0]) == 0
    # a table that is not 16-byte aligned is refused by the build
    dev.tab[1] = be.ptr(dev.tables[1]) + 4
    assert dev.build(fill='noise') == UNSUPPORTED
    np.testing.assert_array_equal(be.get(dev.desc), np.resize(FILLS['noise'], dev.desc_bytes))
    dev.tab[1] = None
    assert dev.build(fill='noise') == INVALID


@pytest.mark.parametrize('qt', ['1-chain', '2-inter'])
def test_no_queries(be, qt):
    prob = problem(qt, 48, 2, (), 43)
    assert prob.Q == 0 and prob.n == 0
    dev = Device(be, prob)
    assert dev.build() == OK
    assert be.lib.mpqe_rgcn_mixed_workspace_bytes(prob.qid, 0, 48) == 0
    for embed in (False, True):
        st, _ = dev.mixed(embed=embed, ws=None)
        assert st == OK and int(be.get(dev.err)[0]) == 0
    assert_fence_intact(be, dev.desc, 'descriptors')


@pytest.mark.parametrize('readout', ['mp', 'sum'])
def test_embed_then_the_plain_score_ops(be, readout):
    """mpqe_rgcn_embed_mixed + mpqe_embed_l2norm_fwd + mpqe_cosine_fwd over the whole set = mpqe_rgcn_fwd_mixed (every
    formula's target table is table 0 here, so one plain lookup serves all pairs)"""
    prob = problem('3-chain_inter', 128, 6, RUNS_MAIN, 47, readout=readout, same_target=True)
    dev, want = check(be, prob)
    st, q_out = dev.mixed(embed=True)
    assert st == OK
    ids, qrow = dev.keep[2], dev.keep[3]
    t, s = be.empty((prob.n, prob.D)), be.empty((prob.n,))
    tt = dev.tables[0]
    assert be.lib.mpqe_embed_l2norm_fwd(be.ptr(tt), int(tt.shape[0]), prob.D, be.ptr(dev.node_map), int(dev.node_map.shape[0]),
                                        be.ptr(ids), prob.n, be.ptr(t), prob.D, None, be.ptr(dev.err), be.stream) == OK
    assert be.lib.mpqe_cosine_fwd(be.ptr(q_out), be.ptr(qrow), be.ptr(t), prob.n, prob.D, 1e-8, be.ptr(s), be.stream) == OK
    np.testing.assert_array_equal(bits(be.get(s)), bits(want))
    assert int(be.get(dev.err)[0]) == 0


def test_run_to_run_bits(be):
    prob = problem('3-inter_chain', 48, 6, RUNS_MAIN, 100 * TYPES.index('3-inter_chain') + 48, neg_counts=NEG_FEW)
    dev = Device(be, prob)
    assert dev.build() == OK
    runs = []
    for fill in ('zeros', 'noise'):
        dev.workspace(fill=fill)
        st, scores = dev.mixed()
        assert st == OK
        runs.append(be.get(scores).tobytes())
    assert runs[0] == runs[1]
