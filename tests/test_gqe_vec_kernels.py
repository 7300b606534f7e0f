"""mpqe_gqe_fwd / mpqe_gqe_bwd / mpqe_gqe_embed (csrc/gqe.hip) under the two vector path operators -- programme int [7] = 1
translate (TransE), 2 scale (the diagonal bilinear form), and [27] = 1 the dot score of the diagonal decoder's chains --
through the C ABI against the extended float64 oracle (tests/gqe_vec_oracle.py), on the host emulator and on the GPU (the
`be` fixture of tests/test_gqe_kernels.py).

Tolerances: FWD / BWD of tests/gqe_oracle.py (scores rtol 1e-5 / atol 1e-6, dot scores too; every gradient rtol 1e-4 /
atol 2e-6). Problems come from the first seed for which the oracle alone finds no near-tie and the problem well
conditioned (gqe_vec_common.settled_problem: the rules of gqe_common.settled_problem on the extended oracle), so nothing
is dropped: the 5 % cap is met with 0.
Shapes: D 16 / 48 / 256 (one and three column blocks, and the largest D: every lane holds four floats of the vector),
B 1 / 17 / 33 (a tile tail, more than one workgroup -- and, the vector-gradient reduction owning one partial row per
16-row workgroup (GQ_ROWS in csrc/gqe.hip), two and three partial rows in the intersection forms, up to 19 in the chain
forms, where the P rows are the B + sum(L) targets and negatives), ragged negative lengths 0 .. 20, duplicate ids."""
import copy
import ctypes

import numpy as np
import pytest

from tests import gqe_common as gc
from tests import gqe_vec_common as vc
from tests.fenced import assert_fence_intact, fenced
from tests.gqe_oracle import BWD, FWD
from tests.test_gqe_kernels import INVALID, OK, TYPES, be  # noqa: F401  (`be`: the backend fixture)

DECODERS = ('transe', 'bilinear-diag')
GQ_ROWS = 16            # csrc/gqe.hip: the rows of one workgroup = of one partial row of a vector's gradient

_SETTLED = {}


def settled(dec, qt, D, B, inter):
    """(problem, oracle with gradients, oracle scores): computed once, shared by both backends, left unchanged."""
    key = (dec, qt, D, B, inter)
    if key not in _SETTLED:
        _SETTLED[key] = vc.settled_problem(dec, qt, D, B, inter, 1000 * DECODERS.index(dec) + 100 * TYPES.index(qt) + D + B)
    return _SETTLED[key]


def check(be, prob, o, scores, packed=None):
    call = vc.call(be, prob, packed)
    assert call.forward() == OK
    got = be.get(call.scores)
    print('scores: max abs error %.3g (max |ref| %.3g)' % (np.abs(got - scores).max(), np.abs(scores).max()))
    np.testing.assert_allclose(got, scores, **FWD)
    assert call.backward() == OK
    assert int(be.get(call.err)[0]) == 0
    for k, g in call.grads.items():
        assert g.shape == o.grads[k].shape, k
        print('%s: max abs error %.3g (max |ref| %.3g)' % (k, np.abs(g - o.grads[k]).max(), np.abs(o.grads[k]).max()))
        np.testing.assert_allclose(g, o.grads[k], err_msg=k, **BWD)
    for k, g in o.grads.items():
        assert k in call.grads or not g.any(), k
    return call


def _cases():
    out = []
    for dec in DECODERS:
        for qt in TYPES:
            for D in (16, 48, 256):
                for B in (1, 17, 33):
                    for inter in (('mean', 'min') if 'inter' in qt else ('mean',)):
                        out.append((dec, qt, D, B, inter))
    return out


@pytest.mark.parametrize('dec,qt,D,B,inter', _cases())
def test_forward_backward_against_oracle(be, dec, qt, D, B, inter):
    prob, o, scores = settled(dec, qt, D, B, inter)
    assert prob.near_ties(o) == 0           # the oracle alone drops nothing (cap: 5 %)
    if B > 1:
        assert (prob.neg_lengths == 0).any() and (prob.neg_lengths > 16).any()
        assert (prob.anchors[1] == prob.anchors[0]).all() and prob.targets[B - 1] == prob.targets[0]
    check(be, prob, o, scores)


@pytest.mark.parametrize('dec,inter', [('transe', 'mean-simple'), ('bilinear-diag', 'min-simple')])
def test_simple_intersection(be, dec, inter):
    prob, o, scores = settled(dec, '3-inter', 48, 17, inter)
    check(be, prob, o, scores)


def test_diagonal_chain_scores_are_not_cosines():
    """What the dot-score cases above can tell apart: the oracle's chain scores under the diagonal decoder are no cosines
    (some leave [-1, 1] or differ from the cosine of the same rows by far more than FWD)."""
    prob, o, scores = settled('bilinear-diag', '2-chain', 48, 17, 'mean')
    a, b = o.tape[-1][1]
    cos = scores / (np.linalg.norm(a.v, axis=1) * np.linalg.norm(b.v, axis=1))
    assert np.abs(cos - scores).max() > 1e-2


@pytest.mark.parametrize('dec', DECODERS)
@pytest.mark.parametrize('qt,inter', [('2-chain', 'mean'), ('2-inter', 'min'), ('2-inter', 'min-simple')])
def test_one_relation_at_two_sites(be, dec, qt, inter):
    """r.r in a chain / r & r in an intersection: the ONE vector gets both sites' terms (the oracle adds them; a kernel
    that dropped the second would give half). With the two anchors of every query also the same entity, the two branches
    are EXACT ties of the minimum: the gradient goes to branch 0."""
    def same_anchor(prob):
        prob.anchors[:, -1] = prob.anchors[:, 0]
    prob, o, scores = vc.settled_problem(dec, qt, 48, 17, inter, 7, repeat=True, tweak=same_anchor)
    if 'inter' in qt:
        assert (o.kept['min_gap'] == 0).all()
    call = check(be, prob, o, scores)
    keys = [k for k in call.mat_keys if k.startswith('path_dec.')]
    assert len(keys) == 1 and call.grads[keys[0]].shape == (48,) and call.grads[keys[0]].any()


@pytest.mark.parametrize('dec', DECODERS)
def test_vector_gradient_over_several_partials(be, dec):
    """The reduction owns one partial row per 16-row workgroup (GQ_ROWS). B = 33 in an intersection form: p_rows = 33 ->
    three partial rows, the last of one real row and 15 padded ones. Chain form, B = 17: p_rows = 17 + sum(L) = 108 rows,
    seven partial rows, the last of 12 real rows. (The padded rows are left out of the sum by rule; in this kernel their
    gradient is exactly zero -- nothing is scored against them --, so a sum that took them in would give the same bits:
    no output can tell the two apart, and this test does not claim to.)"""
    for qt, B, rows in (('3-inter', 33, 33), ('2-chain', 17, None)):
        prob, o, scores = settled(dec, qt, 48, B, 'mean')
        call = check(be, prob, o, scores)
        p_rows = call.p_rows
        assert rows is None or p_rows == rows
        assert (p_rows + GQ_ROWS - 1) // GQ_ROWS >= 2 and p_rows % GQ_ROWS != 0


@pytest.mark.parametrize('dec', DECODERS)
def test_run_to_run_bits(be, dec):
    prob, o, scores = settled(dec, '3-inter_chain', 256, 33, 'min')
    prob2, _, _ = settled(dec, '3-chain', 48, 33, 'mean')
    for p in (prob, prob2):
        runs = []
        for _ in range(2):
            call = vc.call(be, p)
            assert call.forward() == OK and call.backward() == OK
            runs.append((be.get(call.scores), call.grads))
        assert runs[0][0].tobytes() == runs[1][0].tobytes()
        for k in runs[0][1]:
            assert runs[0][1][k].tobytes() == runs[1][1][k].tobytes(), k


@pytest.mark.parametrize('dec', DECODERS)
@pytest.mark.parametrize('qt', ['2-chain', '3-inter'])
def test_bad_id_flags_and_spares_the_other_queries(be, dec, qt):
    """One id of no mode: the error word is set, every result is finite and the other queries' scores are those of the
    clean call to the bit. (The bad row becomes zeros BEFORE the sites: translated by v it is not zero, so unlike on the
    bilinear path its score is whatever v scores -- finite, and of that query alone.)"""
    prob, o, scores = settled(dec, qt, 48, 17, 'mean')
    clean = vc.call(be, prob)
    assert clean.forward() == OK
    want = be.get(clean.scores)
    prog, modes, mats, p_ids, e_ids, qrow, neg_off = vc.pack(prob)
    victim = 5
    bad = prob.node_map.shape[0] - 1              # (in the map, of no mode: -1)
    if qt == '2-chain':
        p_ids = p_ids.copy()
        p_ids[0, victim] = bad                    # the target of query 5: a P row, the one the sites move
    else:
        p_ids = p_ids.copy()
        p_ids[0, victim] = bad
    call = vc.call(be, prob, (prog, modes, mats, p_ids, e_ids, qrow, neg_off))
    assert call.forward() == OK
    assert int(be.get(call.err)[0]) & 1
    got = be.get(call.scores)
    q_of = np.concatenate([np.arange(prob.B), np.repeat(np.arange(prob.B), prob.neg_lengths)])
    keep = (q_of != victim) if qt != '2-chain' else (np.arange(prob.n) != victim)
    assert np.isfinite(got).all()
    np.testing.assert_array_equal(got[keep], want[keep])
    assert call.backward() == OK
    for g in call.grads.values():
        assert np.isfinite(g).all()


# ---------------------------------------------------------------------------------------------- fences, alignment, statuses
class FencedCall(gc.Call):
    """gc.Call with every [D] parameter and its gradient between NaN fences (tests/fenced.py), `misalign` floats off a
    16-byte boundary."""

    def __init__(self, be, prob, misalign=0, misalign_grad=0):
        super(FencedCall, self).__init__(be, prob, vc.pack(prob))
        self.misalign_grad = misalign_grad
        self.mats = [fenced(be, prob.params[k], misalign if prob.params[k].ndim == 1 else 0) for k in self.mat_keys]

    def backward(self):
        be = self.be
        gs = be.put(self.prob.grad_scores)
        self.gtabs = [be.zeros(tuple(t.shape), np.float32) for t in self.tables]
        self.gmats = [fenced(be, np.zeros(tuple(m.shape), np.float32), self.misalign_grad if len(m.shape) == 1 else 0)
                      for m in self.mats]
        gt = (ctypes.c_void_p * len(self.gtabs))(*[be.ptr(g) for g in self.gtabs])
        gm = (ctypes.c_void_p * max(len(self.gmats), 1))(*[be.ptr(g) for g in self.gmats])
        st = be.lib.mpqe_gqe_bwd(*(self._common() + (be.ptr(gs), gt, gm, self.wp, self.wb, be.ptr(self.err), be.stream)))
        self.grads = {}
        for m, g in zip(self.modes, self.gtabs):
            self.grads['enc.feat-%s.weight' % m] = be.get(g)
        for k, g in zip(self.mat_keys, self.gmats):
            self.grads[k] = be.get(g)
        return st


@pytest.mark.parametrize('dec', DECODERS)
@pytest.mark.parametrize('qt,inter', [('3-chain', 'mean'), ('3-inter_chain', 'min'), ('3-chain_inter', 'mean')])
def test_vectors_between_fences(be, dec, qt, inter):
    """A site that read its vector as a [D, D] matrix would meet the NaN fence (scores and gradients NaN); one that wrote
    D * D gradient floats would overwrite it."""
    prob, o, scores = settled(dec, qt, 48, 17, inter)
    call = FencedCall(be, prob)
    assert call.forward() == OK
    np.testing.assert_allclose(be.get(call.scores), scores, **FWD)
    assert call.backward() == OK
    nvec = 0
    for k, g in call.grads.items():
        np.testing.assert_allclose(g, o.grads[k], err_msg=k, **BWD)
    for k, m, g in zip(call.mat_keys, call.mats, call.gmats):
        assert_fence_intact(be, m, k)
        assert_fence_intact(be, g, 'grad ' + k)
        nvec += len(m.shape) == 1
    assert nvec >= 2


@pytest.mark.parametrize('dec', DECODERS)
def test_vector_off_a_16_byte_boundary_is_refused(be, dec):
    prob, o, scores = settled(dec, '2-chain', 48, 17, 'mean')
    call = FencedCall(be, prob, misalign=1)
    assert call.forward() == INVALID
    call = FencedCall(be, prob, misalign_grad=1)
    assert call.forward() == OK
    assert call.backward() == INVALID
    for g in call.gmats:
        assert_fence_intact(be, g)
        assert not be.get(g).any()            # (refused before any launch)


def test_statuses(be):
    prob, o, scores = settled('transe', '2-chain', 48, 17, 'mean')
    packed = list(vc.pack(prob))

    def status(edit=None, num_mats=None):
        call = vc.call(be, prob, tuple(packed))
        if edit:                                   # (after the constructor, which sizes the workspace from the programme)
            call.prog = packed[0].copy()
            edit(call.prog)
        if num_mats is not None:
            common = call._common

            def cut():
                c = list(common())
                c[7] = num_mats
                return tuple(c)
            call._common = cut
        st = call.forward()
        assert np.isnan(be.get(call.scores)).all() or st == OK        # (refused: nothing was launched)
        return st

    def set_(i, v):
        def f(prog):
            prog[i] = v
        return f
    assert status() == OK
    assert status(set_(7, 3)) == INVALID and status(set_(7, -1)) == INVALID
    assert status(set_(27, 2)) == INVALID and status(set_(27, -2)) == INVALID
    assert status(set_(27, 1)) == OK                # (translate sites with the dot score: a legal programme)
    assert status(num_mats=1) == INVALID            # the programme names vector 1
    wb = be.lib.mpqe_gqe_workspace_bytes
    assert wb(packed[0].ctypes.data, 17, 17, 48) > 0
    bad = packed[0].copy()
    bad[7] = 3
    assert wb(bad.ctypes.data, 17, 17, 48) == 0
    # translate sites keep no X and no dY: less workspace than the matrix programme of the same sizes
    mat = packed[0].copy()
    mat[7] = 0
    scale = packed[0].copy()
    scale[7] = 2
    n = prob.n
    assert wb(packed[0].ctypes.data, n, n, 48) < wb(scale.ctypes.data, n, n, 48) < wb(mat.ctypes.data, n, n, 48)


def _scored_rows_offset(dec, sites, p_rows, D):
    """Where a chain programme's saved scored rows start in the workspace, in floats (the plan of csrc/gqe.hip: per vector
    site X [Rp16, D] under scale only, then one partial row per workgroup rounded up to 64 floats; then the scored rows)."""
    rp16 = (p_rows + GQ_ROWS - 1) // GQ_ROWS * GQ_ROWS
    part = (rp16 // GQ_ROWS * D + 63) // 64 * 64
    return sites * (part + (rp16 * D if dec == 'bilinear-diag' else 0))


@pytest.mark.parametrize('dec', DECODERS)
@pytest.mark.parametrize('qt', ['1-chain', '3-chain'])
def test_embed_without_ids_gives_the_forward_s_scored_rows(be, dec, qt):
    """mpqe_gqe_embed with p_ids == NULL (a whole table through the chain, as answer() projects its candidates): row r is,
    to the bit, the row the forward scores for an id of table row r (read from the states the forward saves), and the
    call with ids gives the same bits."""
    prob, o, scores = settled(dec, qt, 48, 17, 'mean')
    prog, modes, mats, p_ids, e_ids, qrow, neg_off = vc.pack(prob)
    table = prob.params['enc.feat-%s.weight' % modes[0]]
    rows = table.shape[0] - 1
    ids = prob.ids[prob.formula.target_mode][:rows]                 # ids whose rows are 0 .. rows - 1, in order
    assert (prob.node_map[ids] == np.arange(rows)).all()
    whole = copy.copy(prob)                         # (the same parameters; one scored pair per table row)
    whole.n = rows
    call = gc.Call(be, whole, (prog, modes, mats, ids.reshape(1, -1), e_ids[:1], np.zeros(rows, dtype=np.int64), None))
    assert call.forward() == OK
    first = (call.wp - be.ptr(call.ws)) // 4 + _scored_rows_offset(dec, len(prob.formula.rels), rows, prob.D)
    scored = be.get(call.ws)[first:first + rows * prob.D].reshape(rows, prob.D)
    c = call._common()
    out = be.empty((rows, prob.D), np.float32)
    assert be.lib.mpqe_gqe_embed(c[0], c[1], c[2], c[3], None, 0, c[6], c[7], c[8], None, rows, be.ptr(out),
                                 be.ptr(call.err), be.stream) == OK
    emb = be.get(out)
    with_ids = be.empty((rows, prob.D), np.float32)
    assert be.lib.mpqe_gqe_embed(c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], c[9], rows, be.ptr(with_ids),
                                 be.ptr(call.err), be.stream) == OK
    assert int(be.get(call.err)[0]) == 0
    assert emb.tobytes() == be.get(with_ids).tobytes()
    assert emb.tobytes() == scored.tobytes()
    want = o.p['enc.feat-%s.weight' % modes[0]][:rows]
    want = want / np.linalg.norm(want, axis=1, keepdims=True)
    for rel in prob.formula.rels:
        v = o.p['path_dec.' + '_'.join(rel)]
        want = want + v if dec == 'transe' else want * v
    np.testing.assert_allclose(emb, want, **FWD)


@pytest.mark.parametrize('dec', DECODERS)
def test_sites_are_applied_one_after_another_to_the_bit(be, dec):
    """Three sites are ((x op v1) op v2) op v3, each result rounded to fp32 -- the reference's op sequence -- not
    x op (v1 op v2 op v3): the embed of a 3-chain equals, bit for bit, numpy float32 applying the three vectors in turn to
    the embed of the same programme with no site at all (the kernel's own normalised rows). fp32 addition and
    multiplication are correctly rounded on both sides, so nothing but the order of the operations can differ; the
    vectors combined first give other bits."""
    prob, o, scores = settled(dec, '3-chain', 48, 17, 'mean')
    prog, modes, mats, p_ids, e_ids, qrow, neg_off = vc.pack(prob)
    call = vc.call(be, prob)
    rows = prob.params['enc.feat-%s.weight' % modes[0]].shape[0] - 1
    c = call._common()

    def embed(prog):
        prog = np.ascontiguousarray(prog, dtype=np.int32)
        out = be.empty((rows, prob.D), np.float32)
        assert be.lib.mpqe_gqe_embed(prog.ctypes.data, c[1], c[2], c[3], None, 0, c[6], c[7], c[8], None, rows, be.ptr(out),
                                     be.ptr(call.err), be.stream) == OK
        return be.get(out)
    bare = prog.copy()
    bare[9] = 0                                     # branch 0: no sites
    x = embed(bare)
    vs = [prob.params['path_dec.' + '_'.join(r)] for r in prob.formula.rels]
    assert len(vs) == 3 and all(v.dtype == np.float32 for v in vs) and x.dtype == np.float32
    step = np.add if dec == 'transe' else np.multiply
    want = step(step(step(x, vs[0]), vs[1]), vs[2])
    assert want.dtype == np.float32
    assert embed(prog).tobytes() == want.tobytes()
    first = step(x, step(step(vs[0], vs[1]), vs[2]))
    assert first.tobytes() != want.tobytes()        # (the other order is another result: the comparison can tell)
