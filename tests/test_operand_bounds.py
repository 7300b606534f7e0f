"""The four entry points of the tile core (csrc/gemm_core.h) with every operand inside fences (tests/fenced.py): the dense
layer, the template and the general R-GCN layer, the ranking kernels.

The other kernel tests hand over private, exactly sized, 16-byte aligned arrays whose surroundings hold finite numbers: a
kernel that reads outside its operand and multiplies the stray value by a zero-filled K column passes them. Here the
surroundings are NaN (integers: a sentinel), so such a read turns the result into NaN, outputs are checked for stray
writes bit for bit, and the scalar load path is reached through a pointer that is 4 bytes off a 16-byte boundary, not only
through odd dims. The ranking kernels also run with several column tiles per strip (the candidate list carried from tile
to tile), which needs more than 64 column tiles.

References: float64 numpy (dense layer, scores) and the CPU oracle of tests/test_kernels.py (R-GCN layers). Tolerances are
the project's own, imported: `close` of tests/test_kernels.py (forward rtol 1e-5, gradients rtol 1e-4, atol 2e-6 * scale)
and `tol` / `check_topk` / `check_rank` of tests/test_rank.py. Every float comparison prints its max abs error.

Runs on the host fiber emulator (`emu`) and on the gfx950 library (`hip`, marked gpu).
"""
import zlib

import numpy as np
import pytest

from mpqe_amd._capi import QUERY_TYPE_IDS
from tests.fenced import assert_fence_intact, fenced
from tests.test_kernels import close, layer_oracle, template_graph
from tests.test_rank import EPS, check_rank, check_topk, csr, make, random_excl, tol, truth


@pytest.fixture(scope='module', params=['emu', pytest.param('hip', marks=pytest.mark.gpu)])
def be(request):
    from tests import kernel_backend
    if request.param == 'emu':
        return kernel_backend.EmuBackend()
    return kernel_backend.HipBackend()


WORST = {}


def check(group, got, ref, rtol=1e-5, scale=None, what=''):
    """Finite, then `close`; prints this comparison's max abs error and the worst of its group so far."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, '%s: shape %s, expected %s' % (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), '%s: %d of %d values are not finite' % (what, (~np.isfinite(got)).sum(), got.size)
    if ref.size:
        err = float(np.abs(got - ref).max())
        WORST[group] = max(WORST.get(group, 0.0), err)
        print('%s / %s: max abs error %.3g (max |ref| %.3g); worst of the group so far %.3g'
              % (group, what, err, np.abs(ref).max(), WORST[group]))
    close(got, ref, rtol=rtol, scale=scale, what=what)


def seed_of(*key):
    return zlib.crc32(repr(key).encode()) % (2 ** 31)       # (the same in every process: hash() of a str is salted)


def nans(*shape):
    return np.full(shape, np.nan, dtype=np.float32)


# ------------------------------------------------------------------------------------------------ dense layer
# (rows, din, dout, pad): W is a column block of a matrix of row stride din + pad, at offset 0, pad / 2 or pad
DENSE_SHAPES = [(70, 48, 20, 16),       # LD_PRED, din % 32 != 0: the loads that ran past the block
                (33, 50, 130, 6),       # odd dims: LD_SCALAR; the middle block is 3 floats (12 bytes) into its row
                (5, 16, 16, 16),
                (65, 40, 64, 24),       # two row tiles, one row in the second
                (64, 32, 64, 32),
                (96, 64, 64, 64),       # LD_FAST throughout
                (80, 64, 64, 64),       # grad_W refuses LD_FAST: rows % 32 != 0
                (257, 96, 60, 32),      # two row chunks of the weight gradient, a ragged second one
                (1, 4, 1, 8)]
BLOCKS = ['first', 'middle', 'last']


def block_offset(pad, block):
    return {'first': 0, 'middle': pad // 2, 'last': pad}[block]


class DenseCase(object):
    """Operands and float64 references of one dense layer on the column block [off, off + din) of a matrix of row stride ld."""

    def __init__(self, rows, din, dout, ld, off, relu, seed):
        rng = np.random.RandomState(seed)
        self.rows, self.din, self.dout, self.ld, self.off, self.relu = rows, din, dout, ld, off, relu
        self.x = rng.randn(rows, din).astype(np.float32)
        self.W = (rng.randn(dout, din) * 0.2).astype(np.float32)
        self.bias = rng.randn(dout).astype(np.float32)
        self.y0 = rng.randn(rows, dout).astype(np.float32)
        self.g = rng.randn(rows, dout).astype(np.float32)
        self.gW0 = rng.randn(dout, din).astype(np.float32)
        self.gb0 = rng.randn(dout).astype(np.float32)
        x64, W64 = self.x.astype(np.float64), self.W.astype(np.float64)
        self.pre = x64 @ W64.T + self.bias.astype(np.float64)

    def y_ref(self, accumulate):
        y = self.pre + (self.y0.astype(np.float64) if accumulate else 0.0)
        return np.maximum(y, 0.0) if self.relu else y

    def grads_ref(self, ymask):
        gpre = self.g.astype(np.float64) * ((ymask > 0) if self.relu else 1.0)
        return gpre @ self.W.astype(np.float64), gpre.T @ self.x.astype(np.float64), gpre.sum(0)


def dense_fwd(be, c, accumulate, mis=()):
    m = lambda name: 1 if name in mis else 0
    x = fenced(be, c.x, m('x'))
    W = fenced(be, c.W, m('W'), ld=c.ld, off=c.off)
    bias = fenced(be, c.bias)
    y = fenced(be, c.y0 if accumulate else nans(c.rows, c.dout), m('y'))
    be.check(be.lib.mpqe_linear_fwd(be.ptr(x), c.rows, be.ptr(W), c.ld, be.ptr(bias), c.din, c.dout, c.relu, accumulate,
                                    be.ptr(y), be.stream), 'linear fwd')
    check('dense forward', be.get(y), c.y_ref(accumulate), what='y (accumulate %d)' % accumulate)
    assert_fence_intact(be, y, 'y')


def dense_bwd(be, c, overwrite, mis=(), want_x=True):
    m = lambda name: 1 if name in mis else 0
    # the mask operand is the reference's own output: a pre-activation within rounding of 0 cannot flip it between the
    # kernel and the reference
    ymask = c.y_ref(0).astype(np.float32)
    ref_x, ref_W, ref_b = c.grads_ref(ymask)
    x = fenced(be, c.x, m('x'))
    W = fenced(be, c.W, m('W'), ld=c.ld, off=c.off)
    y = fenced(be, ymask, m('y'))
    g = fenced(be, c.g, m('grad_y'))
    gx = fenced(be, nans(c.rows, c.din))
    gW = fenced(be, nans(c.dout, c.din) if overwrite else c.gW0, ld=c.ld, off=c.off)
    gb = fenced(be, nans(c.dout) if overwrite else c.gb0)
    wb = be.lib.mpqe_linear_bwd_workspace_bytes(c.rows, c.din, c.dout)
    ws = be.nbytes(wb)
    be.check(be.lib.mpqe_linear_bwd(be.ptr(x), c.rows, be.ptr(W), c.ld, be.ptr(y), be.ptr(g), c.din, c.dout, c.relu,
                                    overwrite, be.ptr(gx) if want_x else None, be.ptr(gW), c.ld, be.ptr(gb), be.ptr(ws),
                                    wb, be.stream), 'linear bwd')
    if want_x:
        check('dense gradients', be.get(gx), ref_x, rtol=1e-4, what='grad_x')
    else:
        assert np.isnan(be.get(gx)).all()
    base_W, base_b = (0.0, 0.0) if overwrite else (c.gW0.astype(np.float64), c.gb0.astype(np.float64))
    check('dense gradients', be.get(gW), base_W + ref_W, rtol=1e-4, what='grad_W (overwrite %d)' % overwrite)
    check('dense gradients', be.get(gb), base_b + ref_b, rtol=1e-4, what='grad_bias (overwrite %d)' % overwrite)
    # grad_W's other column blocks are fence: bit-unchanged
    for t, name in ((gx, 'grad_x'), (gW, 'grad_W'), (gb, 'grad_bias')):
        assert_fence_intact(be, t, name)


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('block', BLOCKS)
@pytest.mark.parametrize('shape', DENSE_SHAPES, ids=lambda s: '%dx%dx%d_pad%d' % s)
def test_dense_layer_column_block_between_nan_blocks(be, shape, block, relu):
    """mpqe_linear_fwd / mpqe_linear_bwd on the first, middle and last column block of a wider matrix whose other blocks,
    like everything around every operand, are NaN: reads must stay inside W[0:dout, 0:din] of the block. Before the
    loader's column bound became the block's width (it was the row stride), the forward cases with din % 32 != 0 and
    ld > din gave non-finite y: the loads ran on into the next block and met the zero-filled tail of x."""
    rows, din, dout, pad = shape
    c = DenseCase(rows, din, dout, din + pad, block_offset(pad, block), relu, seed_of(shape, block, relu))
    for accumulate in (0, 1):
        dense_fwd(be, c, accumulate)
    for overwrite in (1, 0):
        dense_bwd(be, c, overwrite)
    dense_bwd(be, c, 0, want_x=False)           # (accumulate form of Encoder's compress blocks: no grad_x)


@pytest.mark.parametrize('block', BLOCKS)
def test_dense_layer_no_rows_zeroes_its_block_only(be, block):
    """rows = 0: overwrite mode turns the column block of grad_W (and grad_bias) into zeros, accumulate mode changes
    nothing; the block's neighbours stay as they were. (x, y and grad_y hold one row that the call must not look at: an
    empty tensor has no address to hand over.)"""
    din, dout, pad = 48, 20, 16
    c = DenseCase(1, din, dout, din + pad, block_offset(pad, block), 1, 5)
    x, W = fenced(be, nans(1, din)), fenced(be, c.W, ld=c.ld, off=c.off)
    y, g = fenced(be, nans(1, dout)), fenced(be, nans(1, dout))
    gx = fenced(be, nans(1, din))
    gW = fenced(be, nans(dout, din), ld=c.ld, off=c.off)
    gb = fenced(be, nans(dout))
    wb = be.lib.mpqe_linear_bwd_workspace_bytes(0, din, dout)
    ws = be.nbytes(wb)
    be.check(be.lib.mpqe_linear_fwd(be.ptr(x), 0, be.ptr(W), c.ld, None, din, dout, 1, 0, be.ptr(y), be.stream), 'fwd')
    be.check(be.lib.mpqe_linear_bwd(be.ptr(x), 0, be.ptr(W), c.ld, be.ptr(y), be.ptr(g), din, dout, 1, 1, be.ptr(gx),
                                    be.ptr(gW), c.ld, be.ptr(gb), be.ptr(ws), wb, be.stream), 'bwd')
    assert (be.get(gW) == 0).all() and (be.get(gb) == 0).all()
    assert np.isnan(be.get(y)).all() and np.isnan(be.get(gx)).all()
    for t, name in ((y, 'y'), (gx, 'grad_x'), (gW, 'grad_W'), (gb, 'grad_bias')):
        assert_fence_intact(be, t, name)
    # accumulate mode with no rows: nothing changes
    gW2, gb2 = fenced(be, c.gW0, ld=c.ld, off=c.off), fenced(be, c.gb0)
    be.check(be.lib.mpqe_linear_bwd(be.ptr(x), 0, be.ptr(W), c.ld, be.ptr(y), be.ptr(g), din, dout, 1, 0, None,
                                    be.ptr(gW2), c.ld, be.ptr(gb2), be.ptr(ws), wb, be.stream), 'bwd +=')
    np.testing.assert_array_equal(be.get(gW2), c.gW0)
    np.testing.assert_array_equal(be.get(gb2), c.gb0)
    assert_fence_intact(be, gW2, 'grad_W')
    assert_fence_intact(be, gb2, 'grad_bias')


@pytest.mark.parametrize('which', ['x', 'W', 'y', 'grad_y'])
@pytest.mark.parametrize('shape', [(96, 64, 64, 64), (70, 48, 20, 16), (65, 40, 64, 24)],
                         ids=lambda s: '%dx%dx%d_pad%d' % s)
def test_dense_layer_one_operand_one_float_off(be, shape, which):
    """Dims that take the 16-byte paths (LD_FAST, LD_PRED) when everything is aligned; one operand at a time sits 4 bytes
    past a 16-byte boundary, so each term of the host's `vec` conjunction alone sends the call to the scalar path."""
    rows, din, dout, pad = shape
    c = DenseCase(rows, din, dout, din + pad, pad // 2, 1, seed_of(shape, which))
    for accumulate in (0, 1):
        dense_fwd(be, c, accumulate, mis=(which,))
    for overwrite in (1, 0):
        dense_bwd(be, c, overwrite, mis=(which,))


# ------------------------------------------------------------------------------------------------ template layer
MISALIGNED = {'none': (), 'x': ('x',), 'weights': ('basis', 'root'), 'grads': ('out', 'grad_out')}


@pytest.mark.parametrize('mis', list(MISALIGNED))
@pytest.mark.parametrize('shape', [(5, 16, 16, 4), (70, 40, 24, 5), (9, 18, 22, 3), (64, 64, 64, 4)],
                         ids=lambda s: 'B%d_%dx%d' % s[:3])
@pytest.mark.parametrize('qt', ['1-chain', '3-inter', '3-inter_chain'])
def test_template_layer_fenced(be, qt, shape, mis):
    B, Din, Dout, R = shape
    m = lambda name: 1 if name in MISALIGNED[mis] else 0
    qi = QUERY_TYPE_IDS[qt]
    for relu in (0, 1):
        rng = np.random.RandomState(seed_of(qt, shape, relu))
        N, E, ei = template_graph(qt, B)
        x = rng.randn(B * N, Din).astype(np.float32)
        basis = (rng.randn(R, Din, Dout) * 0.3).astype(np.float32)
        root = (rng.randn(Din, Dout) * 0.3).astype(np.float32)
        bias = rng.randn(Dout).astype(np.float32)
        et = rng.randint(0, R, size=E).astype(np.int64)
        if E == 3:
            et[2] = et[0]
        gout = rng.randn(B * N, Dout).astype(np.float32)
        ref = layer_oracle(x, ei, np.tile(et, B), basis, root, bias, relu, gout)
        dx, db, dr = fenced(be, x, m('x')), fenced(be, basis, m('basis')), fenced(be, root, m('root'))
        dbi, dg = fenced(be, bias), fenced(be, gout, m('grad_out'))
        out = fenced(be, nans(B * N, Dout), m('out'))
        be.check(be.lib.mpqe_rgcn_template_fwd(qi, B, et.ctypes.data, be.ptr(dx), be.ptr(db), R, be.ptr(dr), be.ptr(dbi),
                                               Din, Dout, relu, be.ptr(out), be.stream), 'fwd')
        check('template forward', be.get(out), ref[0], what='out')
        assert_fence_intact(be, out, 'out')
        # the backward's mask operand is the oracle's output (see dense_bwd)
        dout_ = fenced(be, ref[0], m('out'))
        wsb = be.lib.mpqe_rgcn_template_bwd_workspace_bytes(qi, B, Din, Dout)
        ws = be.nbytes(wsb)
        gb0, gr0, gbi0 = [rng.randn(*s).astype(np.float32) for s in (basis.shape, root.shape, bias.shape)]
        gx, gb, gr, gbi = fenced(be, nans(B * N, Din)), fenced(be, gb0), fenced(be, gr0), fenced(be, gbi0)
        be.check(be.lib.mpqe_rgcn_template_bwd(qi, B, et.ctypes.data, be.ptr(dx), be.ptr(dout_), be.ptr(dg), be.ptr(db),
                                               R, be.ptr(dr), Din, Dout, relu, be.ptr(gx), be.ptr(gb), be.ptr(gr),
                                               be.ptr(gbi), be.ptr(ws), wsb, be.stream), 'bwd')
        check('template gradients', be.get(gx), ref[1], rtol=1e-4, what='grad_x')
        for got, g0, r, name in ((gb, gb0, ref[2], 'grad_basis'), (gr, gr0, ref[3], 'grad_root'),
                                 (gbi, gbi0, ref[4], 'grad_bias')):
            check('template gradients', be.get(got).astype(np.float64) - g0, r, rtol=1e-4,
                  scale=max(1.0, np.abs(r).max() + np.abs(g0).max()), what=name)
        for t, name in ((gx, 'grad_x'), (gb, 'grad_basis'), (gr, 'grad_root'), (gbi, 'grad_bias')):
            assert_fence_intact(be, t, name)


# ------------------------------------------------------------------------------------------------ general layer
def heavy_graph(rng, Nn, E):
    """test_general_layer_heavy_relation_and_odd_dims' graph at (Nn, E): relation 0 with more than 256 edges (several K
    chunks), relation 1 without an edge, many edges into one node."""
    src, dst = rng.randint(0, Nn, size=E), rng.randint(0, Nn, size=E)
    dst[:E * 2 // 7] = 3
    et = np.zeros(E, dtype=np.int64)
    et[E * 6 // 7:] = 2
    return np.stack([src, dst]).astype(np.int64), et, 3


def register_graph(rng, Nn, E):
    """test_general_layer_dims_of_64_register_tiles' graph at (Nn, E): a ragged last K chunk, relation 2 without an edge."""
    src, dst = rng.randint(0, Nn, size=E), rng.randint(0, Nn, size=E)
    dst[:E * 3 // 22] = 7
    et = rng.choice([0, 1, 3, 4], size=E, p=[0.6, 0.2, 0.15, 0.05]).astype(np.int64)
    return np.stack([src, dst]).astype(np.int64), et, 5


GENERAL = {'heavy_10x6': (heavy_graph, 10, 6),              # odd dims: LD_SCALAR
           'heavy_40x24': (heavy_graph, 40, 24),            # LD_PRED
           'register_128x64': (register_graph, 128, 64)}    # the register-operand kernels when everything is aligned


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('mis', ['none', 'x', 'grad_out', 'basis'])
@pytest.mark.parametrize('case', list(GENERAL))
def test_general_layer_fenced(be, case, mis, relu):
    """mpqe_rgcn_general_fwd / bwd with every operand fenced. With everything aligned and dims of 64 the register-operand
    kernels run (and the backward may run on the bit mask alone, without `out`); with x, grad_out or basis one float off
    the library must fall back to the LDS-staged scalar loads and still be right. Overwrite and accumulate mode."""
    graph, Din, Dout = GENERAL[case]
    Nn, E = 130, 400
    rng = np.random.RandomState(seed_of(case, relu))
    ei, et, R = graph(rng, Nn, E)
    x = rng.randn(Nn, Din).astype(np.float32)
    basis = (rng.randn(R, Din, Dout) * 0.2).astype(np.float32)
    root = (rng.randn(Din, Dout) * 0.2).astype(np.float32)
    bias = rng.randn(Dout).astype(np.float32)
    gout = rng.randn(Nn, Dout).astype(np.float32)
    ref = layer_oracle(x, ei, et, basis, root, bias, relu, gout)
    m = lambda name: 1 if name == mis else 0

    err = be.zeros((1,), np.int32)
    pb, pw = be.lib.mpqe_rgcn_plan_bytes(Nn, E, R), be.lib.mpqe_rgcn_plan_workspace_bytes(Nn, E, R)
    plan, pws = be.nbytes(pb), be.nbytes(pw)
    dei, det = fenced(be, ei), fenced(be, et)
    be.check(be.lib.mpqe_rgcn_plan_build(be.ptr(dei), be.ptr(det), Nn, E, R, be.ptr(plan), pb, be.ptr(pws), pw,
                                         be.ptr(err), be.stream), 'plan')
    dx, db, dr = fenced(be, x, m('x')), fenced(be, basis, m('basis')), fenced(be, root)
    dbi, dg = fenced(be, bias), fenced(be, gout, m('grad_out'))
    out = fenced(be, nans(Nn, Dout))
    mb = be.lib.mpqe_rgcn_general_mask_bytes(Nn, Dout) if relu else 0
    assert (mb > 0) == (relu == 1 and Dout % 64 == 0)
    mbits = fenced(be, np.zeros(mb // 8, dtype=np.int64)) if mb else None
    wf = be.lib.mpqe_rgcn_general_workspace_bytes(Nn, E, R, Din, Dout, 0)
    ws = be.nbytes(wf)
    be.check(be.lib.mpqe_rgcn_general_fwd(be.ptr(plan), Nn, E, R, be.ptr(dx), be.ptr(db), be.ptr(dr), be.ptr(dbi), Din,
                                          Dout, relu, be.ptr(out), be.ptr(mbits), be.ptr(ws), wf, be.stream), 'fwd')
    assert int(be.get(err)[0]) == 0
    check('general forward', be.get(out), ref[0], what='out')
    assert_fence_intact(be, out, 'out')
    if mbits is not None:
        assert_fence_intact(be, mbits, 'relu_mask')
        words = be.get(mbits).view(np.uint64).reshape(Nn, Dout // 64)
        bits = (words[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)
        np.testing.assert_array_equal(bits.reshape(Nn, Dout).astype(bool), be.get(out) > 0)

    wb = be.lib.mpqe_rgcn_general_workspace_bytes(Nn, E, R, Din, Dout, 1)
    ws2 = be.nbytes(wb)
    # `out` may stay away only when the register-operand kernels run: the bit-mask route
    bits_only = mbits is not None and Din % 64 == 0 and mis == 'none'
    gb0, gr0, gbi0 = [rng.randn(*s).astype(np.float32) for s in (basis.shape, root.shape, bias.shape)]
    for overwrite in (1, 0):
        gx = fenced(be, nans(Nn, Din))
        gb, gr, gbi = [fenced(be, nans(*a.shape) if overwrite else a) for a in (gb0, gr0, gbi0)]
        # (accumulate call: `out` alone, the library makes the mask words itself where it wants them)
        p_out = None if (bits_only and overwrite) else be.ptr(out)
        p_bits = be.ptr(mbits) if overwrite else None
        be.check(be.lib.mpqe_rgcn_general_bwd(be.ptr(plan), Nn, E, R, be.ptr(dx), p_out, p_bits, be.ptr(dg), be.ptr(db),
                                              be.ptr(dr), Din, Dout, relu, overwrite, be.ptr(gx), be.ptr(gb), be.ptr(gr),
                                              be.ptr(gbi), be.ptr(ws2), wb, be.stream), 'bwd (overwrite %d)' % overwrite)
        check('general gradients', be.get(gx), ref[1], rtol=1e-4, what='grad_x')
        for got, g0, r, name in ((gb, gb0, ref[2], 'grad_basis'), (gr, gr0, ref[3], 'grad_root'),
                                 (gbi, gbi0, ref[4], 'grad_bias')):
            if overwrite:
                check('general gradients', be.get(got), r, rtol=1e-4, what=name)
            else:
                check('general gradients', be.get(got).astype(np.float64) - g0, r, rtol=1e-4,
                      scale=max(1.0, np.abs(r).max() + np.abs(g0).max()), what=name + ' (accumulate)')
        for t, name in ((gx, 'grad_x'), (gb, 'grad_basis'), (gr, 'grad_root'), (gbi, 'grad_bias')):
            assert_fence_intact(be, t, name)


# ------------------------------------------------------------------------------------------------ ranking
def run_rank(be, q, table, target=None, excl=None, k=0, mis_q=0, mis_t=0):
    """tests/test_rank.py's `run` with every operand and every output inside fences."""
    Q, D = q.shape
    N = table.shape[0]
    dq, dt = fenced(be, q, mis_q), fenced(be, table, mis_t)
    dtarget = None if target is None else fenced(be, np.asarray(target, dtype=np.int64))
    off = rows = None
    E = 0
    if excl is not None:
        o, r = csr(excl, Q)
        E = int(r.shape[0])
        off, rows = fenced(be, o), fenced(be, r if E else np.zeros(1, dtype=np.int64))
    topr = fenced(be, np.full((Q, k), -7, dtype=np.int64)) if k > 0 else None
    tops = fenced(be, nans(Q, k)) if k > 0 else None
    rank = fenced(be, np.full((Q,), -7, dtype=np.int64)) if target is not None else None
    tsc = fenced(be, nans(Q)) if target is not None else None
    need = be.lib.mpqe_rank_workspace_bytes(Q, N, D, k)
    ws = be.nbytes(need)
    err = be.zeros((1,), np.int32)
    st = be.lib.mpqe_rank_entities(be.ptr(dq), Q, be.ptr(dt), N, D, EPS, be.ptr(dtarget), be.ptr(off), be.ptr(rows), E, k,
                                   be.ptr(topr), be.ptr(tops), be.ptr(rank), be.ptr(tsc), be.ptr(ws), need, be.ptr(err),
                                   be.stream)
    assert st == 0, 'status %d' % st
    for t, name in ((topr, 'topk_rows'), (tops, 'topk_scores'), (rank, 'rank'), (tsc, 'target_scores')):
        if t is not None:
            assert_fence_intact(be, t, name)
    get = lambda a: None if a is None else be.get(a)
    return {'rows': get(topr), 'scores': get(tops), 'rank': get(rank), 'tscore': get(tsc), 'err': int(be.get(err)[0])}


def check_ranking(out, s64, target, excl, k, what):
    assert out['err'] == 0
    check_topk(out, s64, excl, k)
    check_rank(out, s64, target, excl)
    Q = s64.shape[0]
    assert np.isfinite(out['tscore']).all()
    worst = float(np.abs(out['tscore'] - s64[np.arange(Q), target]).max())
    for i in range(Q):
        got = out['rows'][i]
        got = got[got >= 0]
        assert np.isfinite(out['scores'][i, :got.size]).all()
        if got.size:
            worst = max(worst, float(np.abs(out['scores'][i, :got.size] - s64[i, got]).max()))
    WORST['ranking'] = max(WORST.get('ranking', 0.0), worst)
    print('ranking / %s: max abs score error %.3g (tol at |s| = 1: %.3g); worst of the group so far %.3g'
          % (what, worst, tol(1.0), WORST['ranking']))


# (5, 63, 10, 3): LD_SCALAR by its dim; (67, 700, 48, 10), (9, 130, 20, 17): LD_PRED when aligned; (9, 130, 32, 5): LD_FAST
# when aligned
@pytest.mark.parametrize('mis', [(0, 0), (1, 0), (0, 1)], ids=['aligned', 'q_off', 'table_off'])
@pytest.mark.parametrize('shape', [(5, 63, 10, 3), (67, 700, 48, 10), (9, 130, 20, 17), (9, 130, 32, 5)],
                         ids=lambda s: 'Q%d_N%d_D%d_k%d' % s)
def test_rank_fenced_and_misaligned(be, shape, mis):
    Q, N, D, k = shape
    rng, q, table, target = make(300 + Q + D, Q, N, D)
    s64 = truth(q, table)
    out = run_rank(be, q, table, target, None, k, *mis)
    check_ranking(out, s64, target, None, k, 'plain')
    excl = random_excl(rng, Q, N, target, 40)
    out = run_rank(be, q, table, target, excl, k, *mis)
    check_ranking(out, s64, target, excl, k, 'exclusions')


# (5, 4161, 16, 10): 66 column tiles, 2 per strip; (3, 8300, 8, .): 130 tiles, 3 per strip, 44 strips; k = 70: the 128-entry
# list variant
@pytest.mark.parametrize('with_excl', [False, True], ids=['plain', 'exclusions'])
@pytest.mark.parametrize('shape', [(5, 4161, 16, 10), (3, 8300, 8, 20), (3, 8300, 8, 70)],
                         ids=lambda s: 'Q%d_N%d_D%d_k%d' % s)
def test_rank_several_tiles_per_strip(be, shape, with_excl):
    """More than 64 column tiles: a workgroup walks several tiles and carries each query's candidate list from one to the
    next (the `full` / threshold early reject, the rule that a newcomer must beat the k-th entry strictly)."""
    Q, N, D, k = shape
    rng, q, table, target = make(400 + N + k, Q, N, D)
    excl = random_excl(rng, Q, N, target, 60) if with_excl else None
    out = run_rank(be, q, table, target, excl, k)
    check_ranking(out, truth(q, table), target, excl, k, 'N %d k %d' % (N, k))


def test_rank_exact_ties_across_the_tiles_of_a_strip(be):
    """tests/test_rank.py's test_constructed_exact_ties with the copies spread over one strip's tiles. N = 4161: strips of
    two 64-row tiles, strip 5 = rows 640..703 and 704..767, three copies in the first and two in the second; one more copy
    sits in a later strip (the merge's tie rule)."""
    Q, N, D, k = 6, 4161, 16, 10
    rng, q, table, _ = make(13, Q, N, D)
    group = [650, 660, 700, 710, 760, 3000]             # all copies of row 650's direction
    for r, f in zip(group[1:], (1.0, 2.0, 0.5, 4.0, 0.25)):
        table[r] = table[650] * np.float32(f)
    for i in range(Q):                                  # the group is every query's best direction among the 4161 rows
        q[i] = (table[650] + np.float32(0.05) * q[i]) * np.float32(2.0 ** -i)
    order = sorted(group)
    for t in (650, 710, 3000):                          # a target in the strip's first tile, in its second, in a later strip
        target = np.full(Q, t, dtype=np.int64)
        out = run_rank(be, q, table, target, None, k)
        for i in range(Q):
            # the tied rows lead, the smaller row first, with bit-equal scores; the rank counts only the smaller ones
            assert out['rows'][i, :len(order)].tolist() == order, 'query %d: %s' % (i, out['rows'][i])
            assert len(set(out['scores'][i, :len(order)].view(np.int32).tolist())) == 1, 'tied rows have bit-equal scores'
            assert out['scores'][i, len(order)] < out['scores'][i, 0]
            assert out['rank'][i] == 1 + order.index(t)
        if order.index(t) > 0:      # excluding a smaller tied row moves the target up by exactly one
            out2 = run_rank(be, q, table, target, [[order[0]]] * Q, k)
            assert (out2['rank'] == order.index(t)).all()
            assert all(out2['rows'][i, :len(order) - 1].tolist() == order[1:] for i in range(Q))
    # k = 2: the list is full of tied rows two rows into the group; the equal rows that follow in the same tile, in the
    # strip's second tile and in the later strip must not displace them
    target = np.full(Q, 710, dtype=np.int64)
    out = run_rank(be, q, table, target, None, 2)
    assert all(out['rows'][i].tolist() == order[:2] for i in range(Q)), out['rows']
    assert (out['scores'][:, 0].view(np.int32) == out['scores'][:, 1].view(np.int32)).all()
    assert (out['rank'] == 4).all()


@pytest.mark.parametrize('shape', [(4, 4161, 16, 10, 2), (3, 8300, 8, 20, 3)], ids=['2_tiles', '3_tiles'])
def test_rank_best_rows_all_in_the_last_tile_of_a_strip(be, shape):
    """Query 0's k best rows all lie in the last tile of strip 7: its list fills in the strip's first tile and is then
    entirely displaced."""
    Q, N, D, k, tps = shape
    rng, q, table, target = make(17 + tps, Q, N, D)
    last = (7 * tps + tps - 1) * 64
    best = last + rng.choice(64, size=k, replace=False)
    for j, r in enumerate(best):        # query 0's direction, less noise for the better rows: k distinct scores near 1
        table[r] = (q[0] * np.float32(1.5) + np.float32(0.01 * (j + 1)) * rng.randn(D)).astype(np.float32)
    s64 = truth(q, table)
    assert set(np.argsort(-s64[0])[:k].tolist()) == set(best.tolist())
    gap = np.sort(s64[0])[::-1]
    assert gap[k - 1] - gap[k] > 4 * tol(1.0), 'the construction separates the k best rows from the rest'
    out = run_rank(be, q, table, target, None, k)
    check_ranking(out, s64, target, None, k, 'last tile, %d per strip' % tps)
    assert set(out['rows'][0].tolist()) == set(best.tolist())
    assert (out['rows'][0] // 64 == 7 * tps + tps - 1).all()


def test_rank_split_calls_are_bit_identical_with_two_tiles_per_strip(be):
    Q, N, D, k = 70, 4161, 16, 12
    rng, q, table, target = make(19, Q, N, D)
    excl = random_excl(rng, Q, N, target, 25)
    a = run_rank(be, q, table, target, excl, k)
    b = run_rank(be, q, table, target, excl, k)
    for key in ('rows', 'rank'):
        np.testing.assert_array_equal(a[key], b[key])
    for key in ('scores', 'tscore'):
        np.testing.assert_array_equal(a[key].view(np.int32), b[key].view(np.int32))
    cut = 33
    lo = run_rank(be, q[:cut], table, target[:cut], excl[:cut], k)
    hi = run_rank(be, q[cut:], table, target[cut:], excl[cut:], k, mis_q=1)     # (and the scalar loads agree to the bit)
    for key in ('rows', 'rank'):
        np.testing.assert_array_equal(a[key], np.concatenate([lo[key], hi[key]]))
    for key in ('scores', 'tscore'):
        np.testing.assert_array_equal(a[key].view(np.int32), np.concatenate([lo[key], hi[key]]).view(np.int32))
