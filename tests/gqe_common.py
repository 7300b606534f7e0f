"""Shared by the GQE tests: fixtures of tests/golden/gqe_*.npz as models / oracles, random problems at other shapes, and
one driver of mpqe_gqe_fwd / mpqe_gqe_bwd through the C ABI for both kernel backends (tests/kernel_backend.py)."""
import ctypes
import os

import numpy as np

from mpqe_amd.graph import Formula
from tests.conftest import CaseGraph, GoldenCase, golden_paths
from tests.gqe_oracle import Oracle

TIE_TOL = 1e-6          # tests/test_configs_gpu.py drop_near_ties: two candidates closer than this are a coin toss in fp32


def case_paths():
    return golden_paths('gqe_')


def case_ids():
    return [os.path.basename(p)[:-4] for p in case_paths()]


def load_case(path):
    return GoldenCase(path)


def case_oracle(case):
    return Oracle({k: v.numpy() for k, v in case.params().items()}, case.arrays['node_map'])


def build_model(case, device=None, fused=True):
    """QueryEncoderDecoder wired like the reference's start-up code (train.py / utils.py), the fixture's parameters loaded
    strictly."""
    from mpqe_amd.data_utils import make_feature_modules
    from mpqe_amd.encoders import DirectEncoder
    from mpqe_amd.model import QueryEncoderDecoder
    from mpqe_amd.utils import get_intersection_decoder, get_metapath_decoder
    feature_modules, node_maps = make_feature_modules(case.ids, case.D, case.num_entities)
    graph = CaseGraph(case)
    enc = DirectEncoder(None, feature_modules, node_maps)
    dims = {m: case.D for m in case.modes}
    model = QueryEncoderDecoder(graph, enc, get_metapath_decoder(graph, dims, 'bilinear'),
                                get_intersection_decoder(graph, dims, case.cfg['inter']))
    model.load_state_dict(case.params(), strict=True)
    model.fused = fused
    return model if device is None else model.to(device)


# ---------------------------------------------------------------------------------------------- random problems
MODES = ('m0', 'm1', 'm2')
NAMES = ('p', 'q')
NEG_CYCLE = (0, 20, 1, 3, 2)          # ragged lengths: a 0 and one above the 16-row tile


def make_formula(query_type, rng, repeat=False):
    """A random formula over MODES x NAMES x MODES; repeat: one relation at two sites (2-chain r.r, 2-inter r & r)."""
    m = lambda: MODES[rng.randint(len(MODES))]       # noqa: E731
    nm = lambda: NAMES[rng.randint(len(NAMES))]      # noqa: E731
    if repeat:
        r = (MODES[0], nm(), MODES[0])
        assert query_type in ('2-chain', '2-inter')
        return Formula(query_type, (r, r))
    if query_type.endswith('chain') and '_' not in query_type:
        k = int(query_type[0])
        ms = [m() for _ in range(k + 1)]
        return Formula(query_type, tuple((ms[i], nm(), ms[i + 1]) for i in range(k)))
    t = m()
    if query_type in ('2-inter', '3-inter'):
        return Formula(query_type, tuple((t, nm(), m()) for _ in range(int(query_type[0]))))
    v = m()
    if query_type == '3-inter_chain':
        return Formula(query_type, ((t, nm(), m()), ((t, nm(), v), (v, nm(), m()))))
    return Formula(query_type, ((t, nm(), v), ((v, nm(), m()), (v, nm(), m()))))


class Problem(object):
    """Random parameters, ids and gradient of the scores for one formula batch, plus its oracle."""

    def __init__(self, query_type, D, B, inter, seed, repeat=False, rows=23):
        rng = np.random.RandomState(seed)
        self.formula = make_formula(query_type, rng, repeat)
        self.D, self.B, self.inter = D, B, inter
        n_ent = rows * len(MODES)
        self.node_map = np.full(n_ent + 1, -1, dtype=np.int64)
        self.ids = {}
        for k, mode in enumerate(MODES):
            self.ids[mode] = np.arange(k, n_ent, len(MODES), dtype=np.int64)
            self.node_map[self.ids[mode]] = np.arange(rows)
        self.params = {}
        for mode in MODES:
            self.params['enc.feat-%s.weight' % mode] = rng.normal(0, 1.0, (rows + 1, D)).astype(np.float32)
        lim = np.sqrt(6.0 / (2 * D))
        for a in MODES:
            for name in NAMES:
                for b in MODES:
                    self.params['path_dec.%s_%s_%s' % (a, name, b)] = rng.uniform(-lim, lim, (D, D)).astype(np.float32)
        for mode in MODES:
            self.params['inter_dec.%s_premat' % mode] = rng.uniform(-lim, lim, (D, D)).astype(np.float32)
            self.params['inter_dec.%s_postmat' % mode] = rng.uniform(-lim, lim, (D, D)).astype(np.float32)
        f = self.formula
        self.anchors = np.stack([rng.choice(self.ids[mode], size=B) for mode in f.anchor_modes], axis=1)
        self.targets = rng.choice(self.ids[f.target_mode], size=B)
        if B > 1:                       # duplicate anchor and target ids: table rows that several entries add into
            self.anchors[1] = self.anchors[0]
            self.targets[B - 1] = self.targets[0]
        self.neg_lengths = np.array([NEG_CYCLE[(i + 1) % len(NEG_CYCLE)] for i in range(B)], dtype=np.int64)
        self.negs = rng.choice(self.ids[f.target_mode], size=int(self.neg_lengths.sum()))
        self.n = B + self.negs.shape[0]
        self.grad_scores = rng.normal(0, 1.0, self.n).astype(np.float32)

    def oracle(self):
        o = Oracle(self.params, self.node_map)
        s = o.forward(self.formula, self.anchors, self.targets, self.negs, self.neg_lengths, self.inter)
        o.backward(self.grad_scores)
        return o, s

    def near_ties(self, o):
        """How many queries hold a coin toss: a minimum decided by less than TIE_TOL between different values, or a ReLU
        input that close to 0 (both discrete choices the fp32 summation order can flip)."""
        bad = np.zeros(self.B, dtype=bool)
        gap = o.kept.get('min_gap')
        if gap is not None:
            bad |= ((gap > 0) & (gap <= TIE_TOL)).any(axis=1)
        for h in o.kept.get('preact', []):
            bad |= (np.abs(h) <= TIE_TOL).any(axis=1)
        return int(bad.sum())


    def well_conditioned(self, o, scores):
        """Whether the tolerances mean anything in fp32 for this problem: the oracle's own op sequence in float32 (numpy,
        BLAS summation order) must stay within HALF of FWD / BWD of the float64 oracle. An intersection whose aggregate
        nearly vanishes (a minimum over ReLUs leaves few, small columns) turns the rounding of its inputs into a direction
        error of the scored vector that no fp32 arithmetic avoids; such a draw cannot test a kernel at these tolerances.
        The criterion reads the oracle alone, never the code under test."""
        from tests.gqe_oracle import BWD, FWD
        o32 = Oracle(self.params, self.node_map, dtype=np.float32)
        s32 = o32.forward(self.formula, self.anchors, self.targets, self.negs, self.neg_lengths, self.inter)
        o32.backward(self.grad_scores)

        def within(a, b, tol):
            return bool((np.abs(a - b) <= 0.5 * (tol['atol'] + tol['rtol'] * np.abs(b))).all())
        return within(s32, scores, FWD) and all(within(o32.grads[k], o.grads[k], BWD) for k in o.grads)


def settled_problem(query_type, D, B, inter, seed, repeat=False, tweak=None):
    """The first seed from `seed` on for which the oracle alone finds no near-tie (so that nothing has to be dropped) and
    the problem well conditioned (Problem.well_conditioned). tweak(prob): edits a problem before it is judged."""
    for s in range(seed, seed + 50):
        prob = Problem(query_type, D, B, inter, s, repeat)
        if tweak is not None:
            tweak(prob)
        o, scores = prob.oracle()
        if prob.near_ties(o) == 0 and prob.well_conditioned(o, scores):
            return prob, o, scores
    raise AssertionError('no seed without near-ties')


def pack(prob):
    """The problem as the arguments of mpqe_gqe_fwd: (prog, modes, matrix keys, p_ids, e_ids, qrow, neg_off)."""
    from mpqe_amd import ops
    from mpqe_amd.model import gqe_plan
    form, branches, imode, tail, emode = gqe_plan(prob.formula)
    modes, mats = [], []

    def table_of(mode):
        if mode not in modes:
            modes.append(mode)
        return modes.index(mode)

    def mat_of(key):
        if key not in mats:
            mats.append(key)
        return mats.index(key)

    pb = [(table_of(m), [(mat_of('path_dec.' + '_'.join(r)), t) for r, t in steps]) for _, m, steps in branches]
    pt = [(mat_of('path_dec.' + '_'.join(r)), t) for r, t in tail]
    pre = post = -1
    if imode is not None and not prob.inter.endswith('simple'):
        pre, post = mat_of('inter_dec.%s_premat' % imode), mat_of('inter_dec.%s_postmat' % imode)
    prog = ops.gqe_programme(form, pb, table_of(emode), prob.inter.split('-')[0], pre, post, pt)
    B = prob.B
    tnodes = np.concatenate([prob.targets, prob.negs]).astype(np.int64)
    qrow = neg_off = None
    if form == 0:
        p_ids, e_ids = tnodes.reshape(1, -1), prob.anchors[:, 0].astype(np.int64)
        qrow = np.concatenate([np.arange(B), np.repeat(np.arange(B), prob.neg_lengths)]).astype(np.int64)
    else:
        p_ids = np.ascontiguousarray(np.stack([prob.anchors[:, slot] for slot, _, _ in branches]).astype(np.int64))
        e_ids = tnodes
        neg_off = np.concatenate([[0], np.cumsum(prob.neg_lengths)]).astype(np.int64)
    return prog, modes, mats, p_ids, e_ids, qrow, neg_off


class Call(object):
    """One forward (+ backward) of a Problem through the C ABI on a backend."""

    def __init__(self, be, prob, packed=None):
        self.be, self.prob = be, prob
        prog, modes, mats, p_ids, e_ids, qrow, neg_off = packed if packed is not None else pack(prob)
        self.prog = np.ascontiguousarray(prog, dtype=np.int32)
        self.modes, self.mat_keys = modes, mats
        self.tables = [be.put(prob.params['enc.feat-%s.weight' % m]) for m in modes]
        self.mats = [be.put(prob.params[k]) for k in mats]
        self.node_map = be.put(prob.node_map)
        self.p_ids, self.e_ids = be.put(p_ids), be.put(e_ids)
        self.qrow = None if qrow is None else be.put(qrow)
        self.neg_off = None if neg_off is None else be.put(neg_off)
        self.p_rows, self.e_rows, self.n = p_ids.shape[1], e_ids.shape[0], prob.n
        self.err = be.zeros(1, np.int32)
        self.wb = be.lib.mpqe_gqe_workspace_bytes(self.prog.ctypes.data, self.p_rows, self.n, prob.D)
        assert self.wb > 0
        self.ws = be.nbytes(self.wb + 256)
        self.wp = (be.ptr(self.ws) + 255) // 256 * 256

    def _common(self):
        be = self.be
        self._tab = (ctypes.c_void_p * len(self.tables))(*[be.ptr(t) for t in self.tables])
        self._rows = (ctypes.c_int64 * len(self.tables))(*[int(t.shape[0]) for t in self.tables])
        self._mat = (ctypes.c_void_p * max(len(self.mats), 1))(*[be.ptr(m) for m in self.mats])
        return (self.prog.ctypes.data, self._tab, self._rows, len(self.tables), be.ptr(self.node_map),
                int(self.node_map.shape[0]), self._mat, len(self.mats), self.prob.D, be.ptr(self.p_ids), self.p_rows,
                be.ptr(self.e_ids), self.e_rows, be.ptr(self.qrow), be.ptr(self.neg_off), self.n, 1e-8)

    def forward(self, save=1):
        be = self.be
        self.scores = be.empty((self.n,), np.float32)
        st = be.lib.mpqe_gqe_fwd(*(self._common() + (save, be.ptr(self.scores), self.wp, self.wb, be.ptr(self.err), be.stream)))
        return st

    def backward(self):
        """-> status; self.grads {parameter key: array}"""
        be = self.be
        gs = be.put(self.prob.grad_scores)
        self.gtabs = [be.zeros(tuple(t.shape), np.float32) for t in self.tables]
        self.gmats = [be.zeros(tuple(m.shape), np.float32) for m in self.mats]
        gt = (ctypes.c_void_p * len(self.gtabs))(*[be.ptr(g) for g in self.gtabs])
        gm = (ctypes.c_void_p * max(len(self.gmats), 1))(*[be.ptr(g) for g in self.gmats])
        st = be.lib.mpqe_gqe_bwd(*(self._common() + (be.ptr(gs), gt, gm, self.wp, self.wb, be.ptr(self.err), be.stream)))
        self.grads = {}
        for m, g in zip(self.modes, self.gtabs):
            self.grads['enc.feat-%s.weight' % m] = be.get(g)
        for k, g in zip(self.mat_keys, self.gmats):
            self.grads[k] = be.get(g)
        return st
