"""The id-independent host decisions of FusedTrainStep.pack (mpqe_amd/fused.py) as pure functions: the launch-form rule,
the lane split, where the touch plan is built, and the template facts they rest on. No GPU: plain Python values and the
library's CPU-side template table."""
import random

import pytest

from mpqe_amd import _capi, ops
from mpqe_amd.fused import _batch_work, chain_form, live_units, split_lanes, touch_mode_for

QUERY_TYPES = ['1-chain', '2-chain', '3-chain', '2-inter', '3-inter', '3-inter_chain', '3-chain_inter']

# query type -> (num anchors, num nodes, [(src, dst)]): reference data_utils.py:325-362. fused.py kept this table beside the
# library's (mpqe_template_info) until it took the library's; the literals live here from now on.
TEMPLATES = {
    '1-chain': (1, 2, [(0, 1)]), '2-chain': (1, 3, [(0, 2), (2, 1)]), '3-chain': (1, 4, [(0, 3), (3, 2), (2, 1)]),
    '2-inter': (2, 3, [(0, 2), (1, 2)]), '3-inter': (3, 4, [(0, 3), (1, 3), (2, 3)]),
    '3-inter_chain': (2, 4, [(0, 2), (1, 3), (3, 2)]), '3-chain_inter': (2, 4, [(0, 3), (1, 3), (3, 2)])}
WORK_PER_GRAPH = {'1-chain': 3, '2-chain': 5, '3-chain': 7, '2-inter': 5, '3-inter': 7, '3-inter_chain': 7,
                  '3-chain_inter': 7}        # edges + nodes


# csrc/step.hip, want_chain: !(flags & MPQE_STEP_NO_CHAIN) && (dim == 64 || dim == 128 || dim == 256); a learned readout:
# num_passes + 1 <= CH_MASK_LEVELS (= 4) for every batch; graphs <= CHAIN_MAX_GRAPHS (= 1 << 20); num_passes <=
# CH_MASK_LEVELS + 1 for every batch.
@pytest.mark.parametrize('flags, dim, learned, graphs, passes, expect', [
    (0, 64, False, 512, 3, True),
    (0, 128, False, 512, 3, True),
    (0, 256, False, 512, 3, True),
    (0, 96, False, 512, 3, False),
    (_capi.STEP_NO_CHAIN, 128, False, 512, 3, False),
    (_capi.STEP_NO_PRUNE | _capi.STEP_NO_KSPLIT, 128, False, 512, 3, True),
    (0, 128, False, 1 << 20, 3, True),
    (0, 128, False, (1 << 20) + 1, 3, False),
    (0, 128, False, 512, 5, True),
    (0, 128, False, 512, 6, False),
    (0, 128, True, 512, 3, True),
    (0, 128, True, 512, 4, False),
])
def test_chain_form_is_want_chain(flags, dim, learned, graphs, passes, expect):
    assert chain_form(flags, dim, learned, graphs, passes) is expect


def test_split_lanes_chain_form_is_one_lane_in_order():
    for nb in (1, 5, 16):
        assert split_lanes(None, [1] * nb, [7] * nb, 4, True) == (list(range(nb)), [0, nb])


# The 11 batches of a bench.py step (synthetic.FULL_MIX at B = 512, adaptive: passes = the formula's diameter).
AIFB_MIX = ['1-chain', '2-chain', '3-chain', '2-inter', '2-inter', '3-inter', '3-inter', '3-inter_chain', '3-inter_chain',
            '3-chain_inter', '3-chain_inter']
AIFB_PASSES = [1, 2, 3, 1, 1, 1, 1, 2, 2, 2, 2]


# Expected values: the lane-split lines of pack() as they stood before split_lanes was cut out of it, run on these inputs.
@pytest.mark.parametrize('lanes, expect', [
    (2, ([1, 2, 4, 6, 9, 0, 3, 5, 7, 8, 10], [0, 5, 11])),
    (3, ([1, 2, 3, 4, 5, 7, 9, 0, 6, 8, 10], [0, 3, 7, 11])),
])
def test_split_lanes_aifb_mix(lanes, expect):
    work = [_batch_work(q, p) for q, p in zip(AIFB_MIX, AIFB_PASSES)]
    assert split_lanes(work, AIFB_PASSES, [512] * 11, lanes, False) == expect


def test_split_lanes_properties():
    rng = random.Random(20240917)
    for _ in range(200):
        nb, lanes = rng.randint(1, 16), rng.randint(1, 4)
        qts = [rng.choice(QUERY_TYPES) for _ in range(nb)]
        passes = [rng.randint(1, 3) for _ in range(nb)]
        sizes = [rng.choice([1, 17, 64, 512, 4096]) for _ in range(nb)]
        work = [_batch_work(q, p) for q, p in zip(qts, passes)]
        order, lane_begin = split_lanes(work, passes, sizes, lanes, False)
        assert sorted(order) == list(range(nb))
        assert lane_begin[0] == 0 and lane_begin[-1] == nb and 1 <= len(lane_begin) - 1 <= min(lanes, nb)
        for lo, hi in zip(lane_begin, lane_begin[1:]):
            assert hi > lo                                            # no empty lane
            assert order[lo:hi] == sorted(order[lo:hi])               # members ascend


T = _capi.TSORT_MAX_ENTRIES


@pytest.mark.parametrize('configured, chain, n_ids, external, in_retry_set, expect', [
    ('step', True, 1000, False, False, 'step'),
    ('step', True, T, False, False, 'step'),
    ('step', True, T + 1, False, False, 'pack'),          # beyond the in-step sort
    ('step', False, 1000, False, False, 'pack'),          # level form
    ('step', False, 1000, True, False, None),             # level form, ids named per run: no plan
    ('step', True, 1000, False, True, 'pack'),            # the in-step plan of this set failed once
    ('pack', True, 1000, False, False, 'pack'),
    (None, False, 1000, False, False, None),              # fp32 atomics
])
def test_touch_mode_for(configured, chain, n_ids, external, in_retry_set, expect):
    assert touch_mode_for(configured, chain, n_ids, external, in_retry_set) == expect


def test_template_facts_are_the_librarys():
    for qt in QUERY_TYPES:
        info = ops.template_info(qt)
        edges = [(info.src[e], info.dst[e]) for e in range(info.num_edges)]
        assert (info.num_anchors, info.num_nodes, edges) == TEMPLATES[qt]
        assert _batch_work(qt, 1) == WORK_PER_GRAPH[qt]
        assert _batch_work(qt, 3) == 3 * WORK_PER_GRAPH[qt]


# live_units(query type, passes, readout, prune, uniform) over passes 1..3 x readout (sum, max, mp) x prune (True, False) x
# uniform (True, False), in that nesting order: the values of the function while it read fused.py's own template table.
LIVE_UNITS = {
    '1-chain': [[2], [3], [2], [3], [2], [3], [2], [3], [1], [2], [2], [3], [2, 3], [3, 3], [2, 3], [3, 3], [2, 3], [3, 3],
                [2, 3], [3, 3], [2, 2], [3, 2], [2, 3], [3, 3], [2, 3, 3], [3, 3, 3], [2, 3, 3], [3, 3, 3], [2, 3, 3],
                [3, 3, 3], [2, 3, 3], [3, 3, 3], [2, 3, 2], [3, 3, 2], [2, 3, 3], [3, 3, 3]],
    '2-chain': [[2], [5], [2], [5], [2], [5], [2], [5], [0], [2], [2], [5], [2, 4], [5, 5], [2, 4], [5, 5], [2, 4], [5, 5],
                [2, 4], [5, 5], [1, 1], [4, 2], [2, 4], [5, 5], [2, 4, 5], [5, 5, 5], [2, 4, 5], [5, 5, 5], [2, 4, 5],
                [5, 5, 5], [2, 4, 5], [5, 5, 5], [2, 3, 2], [5, 4, 2], [2, 4, 5], [5, 5, 5]],
    '3-chain': [[2], [7], [2], [7], [2], [7], [2], [7], [0], [2], [2], [7], [2, 4], [7, 7], [2, 4], [7, 7], [2, 4], [7, 7],
                [2, 4], [7, 7], [0, 0], [4, 2], [2, 4], [7, 7], [2, 4, 6], [7, 7, 7], [2, 4, 6], [7, 7, 7], [2, 4, 6],
                [7, 7, 7], [2, 4, 6], [7, 7, 7], [1, 1, 1], [6, 4, 2], [2, 4, 6], [7, 7, 7]],
    '2-inter': [[4], [5], [4], [5], [4], [5], [4], [5], [2], [3], [4], [5], [4, 5], [5, 5], [4, 5], [5, 5], [4, 5], [5, 5],
                [4, 5], [5, 5], [4, 3], [5, 3], [4, 5], [5, 5], [4, 5, 5], [5, 5, 5], [4, 5, 5], [5, 5, 5], [4, 5, 5],
                [5, 5, 5], [4, 5, 5], [5, 5, 5], [4, 5, 3], [5, 5, 3], [4, 5, 5], [5, 5, 5]],
    '3-inter': [[6], [7], [6], [7], [6], [7], [6], [7], [3], [4], [6], [7], [6, 7], [7, 7], [6, 7], [7, 7], [6, 7], [7, 7],
                [6, 7], [7, 7], [6, 4], [7, 4], [6, 7], [7, 7], [6, 7, 7], [7, 7, 7], [6, 7, 7], [7, 7, 7], [6, 7, 7],
                [7, 7, 7], [6, 7, 7], [7, 7, 7], [6, 7, 4], [7, 7, 4], [6, 7, 7], [7, 7, 7]],
    '3-inter_chain': [[4], [7], [4], [7], [4], [7], [4], [7], [1], [3], [4], [7], [4, 7], [7, 7], [4, 7], [7, 7], [4, 7],
                      [7, 7], [4, 7], [7, 7], [3, 3], [6, 3], [4, 7], [7, 7], [4, 7, 7], [7, 7, 7], [4, 7, 7], [7, 7, 7],
                      [4, 7, 7], [7, 7, 7], [4, 7, 7], [7, 7, 7], [4, 6, 3], [7, 6, 3], [4, 7, 7], [7, 7, 7]],
    '3-chain_inter': [[4], [7], [4], [7], [4], [7], [4], [7], [0], [2], [4], [7], [4, 6], [7, 7], [4, 6], [7, 7], [4, 6],
                      [7, 7], [4, 6], [7, 7], [2, 1], [5, 2], [4, 6], [7, 7], [4, 6, 7], [7, 7, 7], [4, 6, 7], [7, 7, 7],
                      [4, 6, 7], [7, 7, 7], [4, 6, 7], [7, 7, 7], [4, 4, 2], [7, 5, 2], [4, 6, 7], [7, 7, 7]],
}


@pytest.mark.parametrize('qt', QUERY_TYPES)
def test_live_units_unchanged(qt):
    got = [live_units(qt, passes, readout, prune, uniform) for passes in (1, 2, 3) for readout in ('sum', 'max', 'mp')
           for prune in (True, False) for uniform in (True, False)]
    assert got == LIVE_UNITS[qt]
