"""The fused step (mpqe_step_forward_backward) with every operand inside fences (tests/fenced.py), at embedding dimensions
off the tile grid and with operands that are not 16-byte aligned.

tests/test_step.py hands the step private, 16-byte aligned arrays at dimensions that are multiples of four: the scalar
instances of the level kernels, the ragged column tiles, and every host-side choice between a 16-byte and a scalar form are
never exercised there, and a read or write outside an operand meets finite numbers. Here every operand of run_step sits
between NaN fences (integers: a sentinel), so a stray read turns the result into NaN and a stray write is caught bit for
bit, and the groups are
  (a) dimensions off the grid, everything aligned: D = 6 / 33 (LD_SCALAR, the non-vector reduction), 68 / 100 (LD_PRED with a
      ragged second column tile; 256 % (D / 4) != 0), 192 (LD_FAST in the level form, three column tiles), 260 (five columns
      per lane, above the chain form's largest dimension);
  (b) each operand group alone one float (4 bytes) off a 16-byte boundary, then all of them together, at D = 32, 64 (the
      chain form's dimension: a misaligned PARAMETER sends the step to the level form; a misaligned GRADIENT buffer is
      refused, the chain form is chosen before the gradients are known -- and the level form, asked for, takes it) and 68;
      the learned readouts' parameters and gradients likewise;
  (c) the chain form between fences, aligned, so that it stays the chain form;
  (d) the statuses: a touch plan with a misaligned table gradient, a learned readout with D % 4 != 0.

Reference: oracle_step of tests/test_step.py (the CPU oracle's whole model under autograd). Tolerances: the ones
test_fused_step_matches_oracle uses there -- scores and losses rtol 1e-5, atol 1e-6; gradients rtol 1e-4, atol 2e-6. Every
value must be finite before it is compared; every comparison prints its max abs error.

Runs on the host fiber emulator (`emu`) and on the gfx950 library (`hip`, marked gpu).
"""
import functools
import re

import numpy as np
import pytest

from mpqe_amd import _capi
from oracle import ref_cpu
from tests.fenced import assert_fence_intact, fence_bits, fenced
from tests.test_step import EDGE_MIXES, MIXES, _gpu_only_when_heavy, make_problem, oracle_step, run_step


@pytest.fixture(scope='module', params=['emu', pytest.param('hip', marks=pytest.mark.gpu)])
def be(request):
    from tests import kernel_backend
    return kernel_backend.EmuBackend() if request.param == 'emu' else kernel_backend.HipBackend()


SCORE_TOL = dict(rtol=1e-5, atol=1e-6)      # tests/test_step.py: test_fused_step_matches_oracle
GRAD_TOL = dict(rtol=1e-4, atol=2e-6)
MARGIN = 1.0

ALL_MIXES = dict(MIXES, **EDGE_MIXES)
# three batches, one size a multiple of the K step (32) and two that are not: the weight-gradient launch cannot take LD_FAST
ALL_MIXES['ragged3'] = [('3-inter_chain', 33, 1.0), ('2-chain', 1, 0.5), ('1-chain', 32, 0.25)]
# ... and every size a multiple of it (HostPlan.whole_ksteps): LD_FAST weight-gradient tiles at D = 192
ALL_MIXES['whole3'] = [('3-chain_inter', 32, 1.0), ('2-inter', 64, 0.5), ('1-chain', 32, 0.25)]

WORST = {}


class Case(object):
    """A problem of tests/test_step.py: make_problem with the oracle's loss, scores and gradients (computed once, kept)."""

    def __init__(self, seed, D, L, shared, mix, readout, adaptive):
        self.problem = make_problem(seed, D, L, shared, ALL_MIXES[mix], readout, adaptive)
        schema, mode_ids, rel_ids, params, node_map, cfg, batches = self.problem
        self.loss, self.per, self.sp, self.sn = oracle_step(params, cfg, node_map, batches, MARGIN)
        self.grads, seen = {}, set()
        for k, p in params.items():
            if id(p) in seen:
                continue                  # shared layers: one buffer, one accumulated gradient
            seen.add(id(p))
            self.grads[k] = np.zeros(tuple(p.shape), np.float32) if p.grad is None else p.grad.numpy().copy()

    def max_readout_gap(self):
        """The smallest gap between the largest and the second largest final node state of a graph's column, over the whole
        step, from the oracle alone: `max` picks its argument unambiguously only where it is well above rounding."""
        schema, mode_ids, rel_ids, params, node_map, cfg, batches = self.problem
        gap = np.inf
        for b in batches:
            keep = {}
            ref_cpu.encode_queries(params, cfg, node_map, b['formula'], b['col'], keep=keep)
            h = keep['layers'][-1].detach().numpy().astype(np.float64).reshape(b['col']['B'], b['col']['N'], -1)
            top = np.sort(h, axis=1)
            gap = min(gap, float((top[:, -1] - top[:, -2]).min()))
        return gap


@functools.lru_cache(maxsize=None)
def case(seed, D, L, shared, mix, readout, adaptive):
    return Case(seed, D, L, shared, mix, readout, adaptive)


# operand groups of run_step's `place` names
GROUPS = {
    'tables': lambda n: n.startswith('P.enc.feat-'),
    'P.mode_emb': lambda n: n == 'P.mode_embeddings.weight',
    'basis+root': lambda n: re.match(r'P\.layers\.\d+\.(basis|root)$', n) is not None,
    'bias': lambda n: re.match(r'P\.layers\.\d+\.bias$', n) is not None,
    'G.tables': lambda n: n.startswith('G.enc.feat-'),
    'G.mode_emb': lambda n: n == 'G.mode_embeddings.weight',
    'G.basis': lambda n: re.match(r'G\.layers\.\d+\.basis$', n) is not None,
    'G.root': lambda n: re.match(r'G\.layers\.\d+\.root$', n) is not None,
    'G.bias': lambda n: re.match(r'G\.layers\.\d+\.bias$', n) is not None,
    'outputs': lambda n: n in ('loss', 'scores_pos', 'scores_neg'),
    'readout': lambda n: n.startswith('P.readout.') or n.startswith('G.readout.'),
}
ALL = tuple(GROUPS)
WRITTEN = lambda n: n.startswith('G.') or n in ('loss', 'scores_pos', 'scores_neg')


def fenced_step(be, c, mis=(), **kw):
    """run_step with every operand placed by fenced(); the operands of the groups in `mis` one float off a 16-byte boundary.
    Returns run_step's result and {name: (view, initial content)}."""
    placed = {}

    def place(be_, name, array):
        off = 1 if array.dtype.itemsize == 4 and any(GROUPS[g](name) for g in mis) else 0
        placed[name] = (fenced(be_, array, off), np.array(array))
        return placed[name][0]
    try:
        out = run_step(be, *c.problem[:2], *c.problem[3:], MARGIN, place=place, **kw)
    except _capi.MpqeError as e:
        e.placed = placed
        raise
    return out, placed


def close(group, what, got, ref, tol):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, '%s: shape %s, expected %s' % (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), '%s: %d of %d values are not finite' % (what, (~np.isfinite(got)).sum(), got.size)
    err = float(np.abs(got - ref).max()) if ref.size else 0.0
    WORST[group] = max(WORST.get(group, 0.0), err)
    print('%s / %s: max abs error %.3g (max |ref| %.3g); worst of the group so far %.3g'
          % (group, what, err, np.abs(ref).max() if ref.size else 0.0, WORST[group]))
    np.testing.assert_allclose(got, ref, err_msg=what, **tol)


def check(be, group, c, result, placed, backward=True):
    """Loss, scores and every gradient against the oracle; the fences of everything the step writes."""
    loss, sp, sn, grads, err = result
    assert err == 0
    close(group, 'scores_pos', sp, c.sp, SCORE_TOL)
    close(group, 'scores_neg', sn, c.sn, SCORE_TOL)
    close(group, 'loss per batch', loss[1:], c.per, SCORE_TOL)
    close(group, 'loss', loss[0], c.loss, SCORE_TOL)
    for k, ref in c.grads.items():
        if backward:
            close(group, 'grad ' + k, grads[k], ref, GRAD_TOL)
        else:           # a forward-only call leaves the gradient buffers alone, to the bit
            np.testing.assert_array_equal(np.asarray(grads[k]).view(np.int32), placed['G.' + k][1].view(np.int32), err_msg=k)
    written = [n for n in placed if WRITTEN(n)]
    assert len(written) == len(c.grads) + 3
    for name in written:
        assert_fence_intact(be, placed[name][0], name)


def assert_nothing_written(be, placed):
    for name, (view, initial) in placed.items():
        np.testing.assert_array_equal(np.asarray(be.get(view)).view(fence_bits(initial.dtype).dtype),
                                      initial.view(fence_bits(initial.dtype).dtype), err_msg=name)
        assert_fence_intact(be, view, name)


def plan_of(be, capfd, run):
    """run() with the planner's diagnostics on: its result and 'chain' / 'level', the form the plan it made names."""
    be.lib.mpqe_debug_option(b'DUMP_PLAN', 1, 1)
    try:
        capfd.readouterr()
        out = run()
        text = capfd.readouterr().err
    finally:
        be.lib.mpqe_debug_option(b'DUMP_PLAN', 0, 0)
    forms = set(re.findall(r'plan: chain (\d)', text))
    assert len(forms) == 1, text
    return out, 'chain' if forms == {'1'} else 'level'


# ------------------------------------------------------------------------------------------------ (a) dimensions off the grid
READOUTS = {'mp': ('mp', True, 3), 'sum': ('sum', False, 2), 'max': ('max', False, 2)}
OFF_GRID = [(D, 'all7', r) for D in (6, 33, 68) for r in ('mp', 'sum')] + \
           [(D, 'ragged3', r) for D in (100, 192, 260) for r in ('mp', 'sum')] + [(192, 'whole3', 'mp')] + \
           [(6, 'all7', 'max'), (33, 'all7', 'max'), (68, 'all7', 'max'), (100, 'ragged3', 'max'), (260, 'ragged3', 'max')]
# `max`: seeds whose top-2 gap (Case.max_readout_gap) is 2.2e-4, 3.1e-5, 7.7e-6, 1.8e-5 and 3.5e-6 (most seeds draw one entity
# for two anchors of a graph somewhere in the step: two equal node states, a gap of exactly 0)
MAX_SEEDS = {(6, 'all7'): 8, (33, 'all7'): 8, (68, 'all7'): 8, (100, 'ragged3'): 5, (260, 'ragged3'): 1}


@pytest.mark.parametrize('D,mix,readout', OFF_GRID)
def test_dimensions_off_the_tile_grid(be, D, mix, readout):
    """Everything aligned and fenced. `mp` runs with garbage in the gradient buffers (MPQE_STEP_ZERO_GRADS), `sum` and `max`
    accumulate into zeros. `max`: the oracle's top-2 gap of every column of every graph must exceed 1e-6 for the seed used
    (checked on the CPU, from the oracle alone), or the argument of the maximum is a matter of rounding."""
    name, adaptive, L = READOUTS[readout]
    c = case(MAX_SEEDS[(D, mix)] if readout == 'max' else 5, D, L, False, mix, name, adaptive)
    if readout == 'max':
        gap = c.max_readout_gap()
        print('max readout: smallest top-2 gap of the oracle %.3g' % gap)
        assert gap > 1e-6, 'choose another seed: the oracle itself cannot tell the maximum from the runner-up'
    result, placed = fenced_step(be, c, flags=_capi.STEP_ZERO_GRADS if readout == 'mp' else 0)
    check(be, '(a) off-grid D', c, result, placed)


# ------------------------------------------------------------------------------------------------ (b) one float off
MISALIGNED = [g for g in ALL if g != 'readout'] + ['all']
SHAPES_B = [(32, 'all7'), (64, 'fast'), (68, 'all7')]
GRADS_ONLY = ('G.mode_emb', 'G.basis', 'G.root', 'G.bias')


@pytest.mark.parametrize('zero', [False, True], ids=['accumulate', 'zero'])
@pytest.mark.parametrize('group', MISALIGNED)
@pytest.mark.parametrize('D,mix', SHAPES_B)
def test_operand_group_one_float_off(be, capfd, D, mix, group, zero):
    """The level form takes any 4-byte aligned pointer; the chain form 16-byte aligned ones (include/mpqe_amd.h). At D = 64
    the `fast` mix is a chain-form step: a misaligned parameter makes it a level-form step (the planner's diagnostics say
    which form ran); a misaligned gradient buffer alone cannot -- workspace and descriptors were sized for the chain form
    before the gradients were known -- and is refused with nothing written; the same operands pass with MPQE_STEP_NO_CHAIN.
    Entity-table gradients by atomics (touch = False) and the outputs are scalar accesses in both forms. Both ways to deliver
    the gradients: added to what the buffers hold (the reduction reads them) and stored over garbage (MPQE_STEP_ZERO_GRADS:
    the zero fill and the stores)."""
    c = case(11, D, 3, False, mix, 'mp', True)
    mis = tuple(g for g in ALL if g != 'readout') if group == 'all' else (group,)
    flags = _capi.STEP_ZERO_GRADS if zero else 0
    if D == 64 and group in GRADS_ONLY:
        with pytest.raises(_capi.MpqeError, match=r'\(-1\)') as e:
            fenced_step(be, c, mis, touch=False, flags=flags)
        assert_nothing_written(be, {n: v for n, v in e.value.placed.items() if WRITTEN(n)})
        flags |= _capi.STEP_NO_CHAIN
    (result, placed), form = plan_of(be, capfd, lambda: fenced_step(be, c, mis, touch=False, flags=flags))
    if D == 64:
        assert form == ('chain' if group in ('G.tables', 'outputs') else 'level'), group
    else:
        assert form == 'level'
    check(be, '(b) one float off', c, result, placed)


@pytest.mark.parametrize('readout', ['mlp', 'targetmlp'])
@pytest.mark.parametrize('D', [64, 68])
def test_learned_readout_parameters_one_float_off(be, capfd, D, readout):
    """readout_w0 / w2 / b0 / b2 and their gradient buffers one float off: the level form's dense layers pick their scalar
    forms; at D = 64, where the aligned step is a chain-form step, the misaligned one is a level-form step."""
    c = case(23, D, 3, False, 'dup', readout, False)
    (result, placed), form = plan_of(be, capfd, lambda: fenced_step(be, c, ('readout',), touch=False, flags=_capi.STEP_ZERO_GRADS))
    assert form == 'level'
    assert sum(n.startswith('G.readout.') for n in placed) == 4
    check(be, '(b) learned readout one float off', c, result, placed)
    if D == 64:           # ... and aligned it is the chain form, between the same fences
        (result, placed), form = plan_of(be, capfd, lambda: fenced_step(be, c, (), touch=False))
        assert form == 'chain'
        check(be, '(c) chain form', c, result, placed)


# ------------------------------------------------------------------------------------------------ (c) chain form, fenced
CHAIN = [(64, 'mp', 'dup', 'step', 0, 1), (64, 'sum', 'tiny', 'pack', _capi.STEP_ZERO_GRADS, 1),
         (64, 'mp', 'one', False, _capi.STEP_ZERO_GRADS, 1),
         (64, 'mp', 'dup', 'step', _capi.STEP_SPLIT_TAIL | _capi.STEP_ZERO_GRADS, 1),
         (64, 'sum', 'dup', 'pack', _capi.STEP_MERGE_TAIL | _capi.STEP_ZERO_GRADS, 1),
         (64, 'mp', 'dup', 'step', 0, 0),
         (128, 'mp', 'dup', 'step', _capi.STEP_ZERO_GRADS, 1), (128, 'sum', 'tiny', 'step', 0, 1),
         (128, 'mp', 'one', False, 0, 1)]


@pytest.mark.parametrize('D,readout,mix,touch,flags,backward', CHAIN)
def test_chain_form_between_fences(be, capfd, D, readout, mix, touch, flags, backward):
    """Aligned operands between fences: the chain launch, its merged and split tails, the in-step and the pack-time touch
    plan, the atomics form, and a forward-only call, which must leave every gradient buffer as it was."""
    _gpu_only_when_heavy(be, D == 128 and mix == 'dup')
    name, adaptive, L = READOUTS[readout]
    c = case(17, D, L, False, mix, name, adaptive)
    (result, placed), form = plan_of(be, capfd, lambda: fenced_step(be, c, (), touch=touch, flags=flags, backward=backward))
    assert form == 'chain'
    check(be, '(c) chain form', c, result, placed, backward=bool(backward))


# ------------------------------------------------------------------------------------------------ (d) statuses
def test_touch_plan_with_a_misaligned_table_gradient_is_refused(be):
    """The touch plan's table rows are summed and stored in 16-byte pieces: MPQE_ERR_INVALID_ARG, and nothing is written."""
    c = case(17, 64, 3, False, 'tiny', 'mp', True)
    for touch in ('step', 'pack'):
        with pytest.raises(_capi.MpqeError, match=r'\(-1\)') as e:
            fenced_step(be, c, ('G.tables',), touch=touch)
        assert_nothing_written(be, {n: v for n, v in e.value.placed.items() if WRITTEN(n)})


def test_learned_readout_with_an_odd_dimension_is_unsupported(be):
    c = case(23, 6, 2, False, 'tiny', 'mlp', False)
    with pytest.raises(_capi.MpqeError, match=r'\(-2\)') as e:
        fenced_step(be, c, (), touch=False)
    assert_nothing_written(be, {n: v for n, v in e.value.placed.items() if WRITTEN(n)})
