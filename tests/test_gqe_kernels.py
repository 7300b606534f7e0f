"""mpqe_gqe_fwd / mpqe_gqe_bwd (csrc/gqe.hip) through the C ABI against the float64 oracle (tests/gqe_oracle.py), on the
host emulator and on the GPU (the parametrisation of tests/test_kernels.py).

Tolerances: those of the learned-readout parity tests against the oracle in tests/test_configs_gpu.py -- scores rtol 1e-5 /
atol 1e-6, every gradient rtol 1e-4 / atol 2e-6 (restated in tests/gqe_oracle.py as FWD / BWD). A minimum decided by less
than 1e-6 between different values, or a ReLU input that close to 0, is a coin toss in fp32 (drop_near_ties in that file):
every problem here comes from the first seed for which the float64 oracle alone finds none (gqe_common.settled_problem,
checked on the CPU), so nothing is dropped -- the 5 % cap is met with 0. The same search skips draws on which fp32 itself
cannot meet these tolerances (gqe_common.Problem.well_conditioned: the oracle's own op sequence in float32 must stay
within half of them) -- judged from the oracle alone.
Shapes: D 16 / 48 / 128 (one, three and eight column blocks: 48 leaves waves without a block), B 1 / 17 / 33 (a tile
tail, more than one workgroup), ragged negative lengths 0 .. 20 (one above the 16-row tile), duplicate ids; at B 17 also
D 64 (exactly one column block per wave), 80 (wave 0 walks two blocks, the others one) and 256 (the largest D: every lane
holds data, each wave walks four blocks, the static LDS tile is full)."""
import numpy as np
import pytest

from tests import gqe_common as gc
from tests.gqe_oracle import BWD, FWD

TYPES = ['1-chain', '2-chain', '3-chain', '2-inter', '3-inter', '3-inter_chain', '3-chain_inter']
OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3


@pytest.fixture(scope='module', params=['emu', pytest.param('hip', marks=pytest.mark.gpu)])
def be(request):
    from tests import kernel_backend
    if request.param == 'emu':
        return kernel_backend.EmuBackend()
    return kernel_backend.HipBackend()


_SETTLED = {}


def settled(qt, D, B, inter, repeat=False):
    """(problem, oracle with gradients, oracle scores): computed once, shared by both backends, left unchanged."""
    key = (qt, D, B, inter, repeat)
    if key not in _SETTLED:
        _SETTLED[key] = gc.settled_problem(qt, D, B, inter, 100 * TYPES.index(qt) + D + B, repeat)
    return _SETTLED[key]


def check(be, prob, o, scores):
    call = gc.Call(be, prob)
    assert call.forward() == OK
    got = be.get(call.scores)
    err = np.abs(got - scores).max()
    print('scores: max abs error %.3g' % err)
    np.testing.assert_allclose(got, scores, **FWD)
    assert call.backward() == OK
    assert int(be.get(call.err)[0]) == 0
    for k, g in call.grads.items():
        print('%s: max abs error %.3g (max |ref| %.3g)' % (k, np.abs(g - o.grads[k]).max(), np.abs(o.grads[k]).max()))
        np.testing.assert_allclose(g, o.grads[k], err_msg=k, **BWD)
    # (parameters the formula does not use have no gradient on either side)
    for k, g in o.grads.items():
        assert k in call.grads or not g.any(), k
    return call


def _cases():
    out = []
    for qt in TYPES:
        for D in (16, 48, 128):
            for B in (1, 17, 33):
                for inter in (('mean', 'min') if 'inter' in qt else ('mean',)):
                    out.append((qt, D, B, inter))
    for qt in TYPES:
        for D in (64, 80, 256):
            for inter in (('mean', 'min') if 'inter' in qt else ('mean',)):
                out.append((qt, D, 17, inter))
    return out


@pytest.mark.parametrize('qt,D,B,inter', _cases())
def test_forward_backward_against_oracle(be, qt, D, B, inter):
    prob, o, scores = settled(qt, D, B, inter)
    assert prob.near_ties(o) == 0           # the oracle alone drops nothing (cap: 5 %)
    if B > 1:
        assert (prob.neg_lengths == 0).any() and (prob.neg_lengths > 16).any()
        assert (prob.anchors[1] == prob.anchors[0]).all() and prob.targets[B - 1] == prob.targets[0]
    check(be, prob, o, scores)


@pytest.mark.parametrize('inter', ['mean-simple', 'min-simple'])
def test_simple_intersection(be, inter):
    prob, o, scores = settled('3-inter', 48, 17, inter)
    check(be, prob, o, scores)


@pytest.mark.parametrize('qt,inter', [('2-chain', 'mean'), ('2-inter', 'min'), ('2-inter', 'min-simple')])
def test_one_relation_at_two_sites(be, qt, inter):
    """r.r in a chain / r & r in an intersection: the matrix gets both sites' terms. With the two anchors of query 1 also
    the same entity (gc.Problem), that query's two branches are EXACT ties of the minimum: the gradient goes to branch 0."""
    def same_anchor(prob):
        prob.anchors[:, -1] = prob.anchors[:, 0]
    prob, o, scores = gc.settled_problem(qt, 48, 17, inter, 7, repeat=True, tweak=same_anchor)
    if 'inter' in qt:
        assert (o.kept['min_gap'] == 0).all()
    call = check(be, prob, o, scores)
    assert len([k for k in call.mat_keys if k.startswith('path_dec.')]) == 1


def test_run_to_run_bits(be):
    prob, o, scores = settled('3-inter_chain', 128, 33, 'min')
    runs = []
    for _ in range(2):
        call = gc.Call(be, prob)
        assert call.forward() == OK and call.backward() == OK
        runs.append((be.get(call.scores), call.grads))
    assert runs[0][0].tobytes() == runs[1][0].tobytes()
    for k in runs[0][1]:
        assert runs[0][1][k].tobytes() == runs[1][1][k].tobytes(), k


@pytest.mark.parametrize('qt', ['2-chain', '3-inter'])
def test_bad_id_flags_and_spares_the_other_queries(be, qt):
    """One id of no mode: the error word is set, the call returns, and the rows of the other queries are those of the
    clean call."""
    prob, o, scores = settled(qt, 48, 17, 'mean')
    clean = gc.Call(be, prob)
    assert clean.forward() == OK
    want = be.get(clean.scores)
    prog, modes, mats, p_ids, e_ids, qrow, neg_off = gc.pack(prob)
    victim = 5
    bad = prob.node_map.shape[0] - 1              # (in the map, of no mode: -1)
    if qt == '2-chain':
        e_ids = e_ids.copy()
        e_ids[victim] = bad                       # the anchor of query 5
    else:
        p_ids = p_ids.copy()
        p_ids[0, victim] = bad
    call = gc.Call(be, prob, (prog, modes, mats, p_ids, e_ids, qrow, neg_off))
    assert call.forward() == OK
    assert int(be.get(call.err)[0]) & 1
    got = be.get(call.scores)
    q_of = np.concatenate([np.arange(prob.B), np.repeat(np.arange(prob.B), prob.neg_lengths)])
    keep = q_of != victim
    assert np.isfinite(got).all()
    np.testing.assert_array_equal(got[keep], want[keep])
    assert call.backward() == OK                  # (returns; the bad row contributes nothing)
    for g in call.grads.values():
        assert np.isfinite(g).all()
