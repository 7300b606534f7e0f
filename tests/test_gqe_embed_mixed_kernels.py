"""mpqe_gqe_embed_mixed (csrc/gqe.hip) through the C ABI, on the host emulator and on the GPU: the rows mpqe_gqe_fwd_mixed
would score, for queries of DIFFERENT formulas of one intersection type, in one launch.

The oracle is mpqe_gqe_embed on the same backend, handed every run of equal formula alone with its own programme; rows
are compared as uint32 BITS. Problems, fenced operands and the descriptor block are those of tests/test_gqe_mixed_kernels.py
(imported). Shapes: the four intersection types, mean and min, D 16 / 48, B 1 / 16 / 17 / 33 under 1 / 2 / 3 / 5 formulas,
with runs that end before, at and past the 16-row block edges."""
import numpy as np
import pytest

from tests.fenced import assert_fence_intact
from tests.test_gqe_kernels import INVALID, OK, TYPES, WORKSPACE, be  # noqa: F401  (`be`: the backend fixture)
from tests.test_gqe_mixed_kernels import FLAG_BAD_INDEX, Device, bits, place, problem

INTER = ['2-inter', '3-inter', '3-inter_chain', '3-chain_inter']
# B -> (formulas, runs): rows 15 | 16 and 31 | 32 are the block edges
RUNS = {1: (1, ((0, 1),)),
        16: (2, ((0, 9), (1, 7))),                                    # ends exactly at the edge
        17: (3, ((0, 6), (1, 9), (2, 2))),                            # formula 2 holds rows 15 and 16
        33: (5, ((0, 3), (1, 15), (2, 1), (3, 12), (4, 2)))}          # formula 1 crosses row 16, formula 4 row 32


def embed_by_runs(be, dev):
    """the oracle: every run through mpqe_gqe_embed with its own programme -> rows [B, D]"""
    prob = dev.prob
    out = np.zeros((prob.B, prob.D), dtype=np.float32)
    for f, lo, hi in prob.runs():
        p_ids = prob.operands(lo, hi)[0]
        ids = be.put(p_ids)
        rows = be.empty((hi - lo, prob.D), np.float32)
        prog = np.ascontiguousarray(prob.progs[f])
        st = be.lib.mpqe_gqe_embed(prog.ctypes.data, dev.tab, dev.rows, len(dev.tables), be.ptr(dev.node_map),
                                   int(dev.node_map.shape[0]), dev.mat, len(dev.mats), prob.D, be.ptr(ids), hi - lo,
                                   be.ptr(rows), be.ptr(dev.err), be.stream)
        assert st == OK
        out[lo:hi] = be.get(rows)
    return out


def embed_mixed(be, dev, formula_of=None, short=0, prog=None):
    """-> (status, out view [B, D]); the whole problem in one mpqe_gqe_embed_mixed call"""
    prob = dev.prob
    p_ids = prob.operands(0, prob.B)[0]
    fo = place(be, prob.formula_of if formula_of is None else formula_of)
    ids = place(be, p_ids)
    out = place(be, np.full((prob.B, prob.D), np.float32(7.5)))
    prog = np.ascontiguousarray(prob.progs[0] if prog is None else prog)
    st = be.lib.mpqe_gqe_embed_mixed(prog.ctypes.data, prob.F, be.ptr(dev.desc), dev.desc_bytes - short,
                                     be.ptr(dev.node_map), int(dev.node_map.shape[0]), prob.D, be.ptr(fo), prob.B,
                                     be.ptr(ids), be.ptr(out), be.ptr(dev.err), be.stream)
    dev.keep = [fo, ids]
    return st, out


@pytest.mark.parametrize('D', [16, 48])
@pytest.mark.parametrize('inter', ['mean', 'min'])
@pytest.mark.parametrize('qt', INTER)
def test_rows_equal_the_embed_by_runs_to_the_bit(be, qt, inter, D):
    for B, (F, runs) in sorted(RUNS.items()):
        prob = problem(qt, D, F, runs, 300 + 10 * TYPES.index(qt) + B, inter=inter)
        assert prob.B == B and prob.form == 1 and len(prob.runs()) == F
        dev = Device(be, prob)
        want = embed_by_runs(be, dev)
        assert dev.build() == OK
        st, out = embed_mixed(be, dev)
        assert st == OK and int(be.get(dev.err)[0]) == 0
        got = be.get(out)
        assert np.isfinite(want).all()
        np.testing.assert_array_equal(bits(got), bits(want), err_msg='B %d' % B)
        assert_fence_intact(be, out, 'rows')
        assert_fence_intact(be, dev.desc, 'descriptors')


@pytest.mark.parametrize('bad', [-1, 5, 2 ** 40])
def test_bad_formula_index_flags_and_zeroes_its_row(be, bad):
    F, runs = RUNS[33]
    prob = problem('3-inter', 48, F, runs, 300 + 10 * TYPES.index('3-inter') + 33, inter='mean')
    dev = Device(be, prob)
    want = embed_by_runs(be, dev)
    assert dev.build() == OK
    victim = 10                                    # (inside the run that crosses row 16: it is cut in two)
    fo = prob.formula_of.copy()
    fo[victim] = bad
    st, out = embed_mixed(be, dev, formula_of=fo)
    assert st == OK and int(be.get(dev.err)[0]) == FLAG_BAD_INDEX
    got = be.get(out)
    keep = np.arange(prob.B) != victim
    np.testing.assert_array_equal(bits(got[keep]), bits(want[keep]))
    assert (bits(got[victim]) == 0).all()
    assert_fence_intact(be, out, 'rows')


def test_refusals_and_no_queries(be):
    F, runs = RUNS[17]
    prob = problem('2-inter', 16, F, runs, 300 + 10 * TYPES.index('2-inter') + 17, inter='mean')
    dev = Device(be, prob)
    assert dev.build() == OK
    st, out = embed_mixed(be, dev, short=1)
    assert st == WORKSPACE and (be.get(out) == np.float32(7.5)).all()
    chain = problem('2-chain', 16, 2, ((0, 3), (1, 2)), 7)
    st, out = embed_mixed(be, dev, prog=chain.progs[0])             # the chain form goes by runs
    assert st == INVALID and (be.get(out) == np.float32(7.5)).all()
    empty = problem('2-inter', 16, 2, (), 9)
    dev0 = Device(be, empty)
    assert dev0.build() == OK
    st, _ = embed_mixed(be, dev0)
    assert st == OK and int(be.get(dev0.err)[0]) == 0
