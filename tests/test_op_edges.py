"""The per-op kernels of csrc/encoder_ops.hip (embedding gather + L2 norm, variable rows, readouts, scatter_{add,max,mean},
cosine, hinge, LayerNorm + ReLU) and the branch aggregate of csrc/gqe.hip at the edges of their loops: second trips of the
per-lane and per-vector loops, wave and block tails, the alignment fallbacks, signed zeros, exact ties, empty inputs,
addresses that every block hits at once.

Each test runs on the host emulator (`emu`) and on the gfx950 library (`hip`, marked gpu), as in tests/test_kernels.py.
Every expected value is float64 numpy (torch float64 autograd for LayerNorm), formed from the operation's definition in
include/mpqe_amd.h and the kernels' comments; nothing on the expected side comes from the library or from mpqe_amd/ops.py.

Tolerances: `close` of tests/test_kernels.py (forward rtol 1e-5, gradients rtol 1e-4, absolute floor 2e-6 * max(1, max|ref|));
assert_array_equal where the operation is exact (max, argmax, min, masks, copies, hinge gradients). Signed zeros compare by
value (-0.0 == +0.0). Where fp32 atomics add k terms into one address in arbitrary order the bound is the worst case of a
sequential fp32 sum, k * 2^-24 * sum|term| per address. Every float comparison prints its max abs error and max |ref|.

The optimiser steps of csrc/optim.hip close the file: the grid-stride second trip past the capped grid and the scalar path
of unaligned buffers, against torch.optim.Adam / SGD on the CPU with the tolerances of tests/test_kernels.py's optimiser tests.
"""
import numpy as np
import pytest
import torch

from mpqe_amd._capi import FLAG_BAD_INDEX, READOUT_IDS, SCATTER_IDS

U = 2.0 ** -24          # fp32 unit roundoff
EPS = 1e-8              # F.cosine_similarity's clamp
EPS32 = float(np.float32(EPS))          # what the float argument of the C ABI holds


@pytest.fixture(scope='module', params=['emu', pytest.param('hip', marks=pytest.mark.gpu)])
def be(request):
    from tests import kernel_backend
    if request.param == 'emu':
        return kernel_backend.EmuBackend()
    return kernel_backend.HipBackend()


def report(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if b.size:
        with np.errstate(invalid='ignore'):
            print('%s: max abs error %.3g (max |ref| %.3g)' % (what, np.nanmax(np.abs(a - b)), np.abs(b).max()))
    return a, b


def close(a, b, rtol=1e-5, scale=None, what=''):
    a, b = report(a, b, what)
    s = max(1.0, float(np.abs(b).max()) if b.size else 1.0) if scale is None else scale
    np.testing.assert_allclose(a, b, rtol=rtol, atol=2e-6 * s, err_msg=what)


def within(a, b, atol, what=''):
    """|a - b| <= atol, element by element (a derived bound, no relative part)."""
    a, b = report(a, b, what)
    over = np.abs(a - b) > np.broadcast_to(atol, b.shape)
    assert not over.any(), '%s: %d element(s) beyond the bound, first at %s' % (what, over.sum(), np.argwhere(over)[0])


def equal(a, b, what=''):
    """exact, by value: -0.0 == +0.0"""
    np.testing.assert_array_equal(np.asarray(a), np.asarray(b), err_msg=what)


def signs(rng, shape):
    return np.where(rng.rand(*shape) < 0.5, -1.0, 1.0)


# ------------------------------------------------------------------------------------------ scatter
def scatter_ref(op, src, index, size):
    """out, arg (max: the lowest row that attains the maximum, -1 for an empty segment), count. A row whose index lies
    outside 0 .. size-1 belongs to no segment."""
    s = src.astype(np.float64)
    D = s.shape[1]
    out = np.zeros((size, D))
    arg = np.full((size, D), -1, dtype=np.int64)
    count = np.zeros(size)
    for t in range(size):
        rows = np.nonzero(index == t)[0]
        count[t] = len(rows)
        if not len(rows):
            continue
        seg = s[rows]
        if op == 'max':
            out[t] = seg.max(0)
            arg[t] = rows[np.argmax(seg == out[t], axis=0)]
        else:
            out[t] = seg.sum(0) / (len(rows) if op == 'mean' else 1)
    return out, arg, count


def scatter_grad_ref(op, g, index, size, arg, count):
    n, D = len(index), g.shape[1]
    gs = np.zeros((n, D))
    for j in range(n):
        t = index[j]
        if t < 0 or t >= size:
            continue
        if op == 'add':
            gs[j] = g[t]
        elif op == 'mean':
            gs[j] = g[t].astype(np.float64) / max(count[t], 1.0)
        else:
            gs[j] = np.where(arg[t] == j, g[t], 0.0)
    return gs


def run_scatter(be, op, src, index, size, g):
    n, D = src.shape
    wsb = be.lib.mpqe_scatter_workspace_bytes(n, size)
    ws = be.nbytes(wsb)
    out = be.empty((size, D))
    arg = be.empty((size, D), np.int64)
    err = be.zeros((1,), np.int32)
    ds, di = be.put(src), be.put(index)
    be.check(be.lib.mpqe_scatter_fwd(SCATTER_IDS[op], be.ptr(ds), be.ptr(di), n, D, size, be.ptr(out), be.ptr(arg),
                                     be.ptr(ws), wsb, be.ptr(err), be.stream), 'scatter fwd')
    gs = be.empty((n, D))
    dg = be.put(g)
    be.check(be.lib.mpqe_scatter_bwd(SCATTER_IDS[op], be.ptr(dg), be.ptr(di), be.ptr(arg), n, D, size, be.ptr(gs),
                                     be.ptr(ws), wsb, be.stream), 'scatter bwd')
    return be.get(out), be.get(arg), be.get(gs), int(be.get(err)[0])


def check_scatter(be, op, src, index, size, g, sum_atol=None):
    """forward and backward against the float64 definition; sum_atol [D]: the derived bound of a segment that many rows
    hit (for the mean: already divided by the count)."""
    ref, ref_arg, count = scatter_ref(op, src, index, size)
    out, arg, gs, err = run_scatter(be, op, src, index, size, g)
    if op == 'max':
        equal(out, ref, 'max')
        equal(arg, ref_arg, 'arg')
        equal(gs, scatter_grad_ref(op, g, index, size, ref_arg, count), 'grad_src (max)')
    else:
        if sum_atol is None:
            close(out, ref, what='out (%s)' % op)
        else:
            within(out, ref, sum_atol[None, :], 'out (%s)' % op)
        gref = scatter_grad_ref(op, g, index, size, ref_arg, count)
        if op == 'add':
            equal(gs, gref, 'grad_src (add)')
        else:
            close(gs, gref, rtol=1e-4, what='grad_src (mean)')
    return err


ZEROS_SRC = np.array([[-0., -0., 1.], [-1., -2., -0.], [-3., 0., -5.],      # segment 0: rows 0, 1; segment 1: row 2
                      [-0., -0., -0.],                                      # segment 2: nothing but -0.0
                      [0., 0., 0.], [-0., -0., -0.]], dtype=np.float32)     # segment 3: +0.0 (row 4), -0.0 (row 5)
ZEROS_INDEX = np.array([0, 0, 1, 2, 3, 3], dtype=np.int64)


@pytest.mark.parametrize('op', ['add', 'max', 'mean'])
@pytest.mark.parametrize('flip', [False, True], ids=['rows', 'rows-reversed'])
def test_scatter_signed_zeros(be, op, flip):
    """-0.0 is a value like any other: the maximum of {-0.0, -1} is 0, a segment that holds only -0.0 is not empty (arg is
    its row, the gradient reaches it), and among {+0.0, -0.0} the lowest row wins. Segment 4 is empty."""
    src, index = (ZEROS_SRC[::-1].copy(), ZEROS_INDEX[::-1].copy()) if flip else (ZEROS_SRC, ZEROS_INDEX)
    size = 5
    g = np.random.RandomState(1).randn(size, 3).astype(np.float32)
    ref, ref_arg, _ = scatter_ref('max', src, index, size)
    # (the reference itself, spelled out for the rows as given: the issue's case)
    if not flip:
        equal(ref, [[0, 0, 1], [-3, 0, -5], [0, 0, 0], [0, 0, 0], [0, 0, 0]])
        equal(ref_arg, [[0, 0, 0], [2, 2, 2], [3, 3, 3], [4, 4, 4], [-1, -1, -1]])
    else:
        equal(ref_arg[2], [2, 2, 2])                   # the row of the lone -0.0
        equal(ref_arg[3], [0, 0, 0])                   # -0.0 (row 0) before +0.0 (row 1): equal values, the lowest row
    assert check_scatter(be, op, src, index, size, g) == 0


@pytest.mark.parametrize('op', ['add', 'max', 'mean'])
def test_scatter_one_hot_segment(be, op):
    """300 rows, all of segment 0 of 2: every block's atomics land on the same 3 addresses; segment 1 stays empty. The
    column maximum is planted twice, at rows 3 and 200 (different blocks): arg 3, gradient to row 3 alone."""
    rng = np.random.RandomState(17)
    n, D, size = 300, 3, 2
    src = rng.randn(n, D).astype(np.float32)
    src[3] = src[200] = np.float32(5.0) + np.arange(D, dtype=np.float32)
    assert (np.abs(src).max(0) == src[3]).all()
    index = np.zeros(n, dtype=np.int64)
    g = rng.randn(size, D).astype(np.float32)
    # worst case of n fp32 additions in any order: n * u * sum|src| per column; the mean then divides by exactly 300
    bound = n * U * np.abs(src.astype(np.float64)).sum(0)
    assert check_scatter(be, op, src, index, size, g, sum_atol=bound / (n if op == 'mean' else 1)) == 0
    if op == 'max':
        _, ref_arg, _ = scatter_ref(op, src, index, size)
        equal(ref_arg, [[3] * D, [-1] * D])


@pytest.mark.parametrize('op', ['add', 'max', 'mean'])
@pytest.mark.parametrize('D', [1, 300])
def test_scatter_negative_segment_and_row_width(be, op, D):
    """Segment 0 holds negative values only (the unsigned-min branch of the float maximum alone); D = 1, and D = 300
    where one source row spans two blocks. Segment 3 is empty."""
    rng = np.random.RandomState(19 + D)
    n, size = 7, 4
    index = np.array([2, 0, 1, 0, 2, 0, 1], dtype=np.int64)
    src = rng.randn(n, D).astype(np.float32)
    src[index == 0] = -np.abs(src[index == 0]) - np.float32(0.25)
    g = rng.randn(size, D).astype(np.float32)
    assert check_scatter(be, op, src, index, size, g) == 0


@pytest.mark.parametrize('op', ['add', 'max', 'mean'])
def test_scatter_empty_input(be, op):
    D, size = 4, 3
    wsb = be.lib.mpqe_scatter_workspace_bytes(0, size)
    ws = be.nbytes(wsb)
    src, index = be.put(np.zeros((0, D), np.float32)), be.put(np.zeros((0,), np.int64))
    out, arg, err = be.empty((size, D)), be.empty((size, D), np.int64), be.zeros((1,), np.int32)
    be.check(be.lib.mpqe_scatter_fwd(SCATTER_IDS[op], be.ptr(src), be.ptr(index), 0, D, size, be.ptr(out), be.ptr(arg),
                                     be.ptr(ws), wsb, be.ptr(err), be.stream), 'n_src = 0')
    equal(be.get(out), np.zeros((size, D)))
    if op == 'max':
        equal(be.get(arg), np.full((size, D), -1))
    assert int(be.get(err)[0]) == 0
    g, gs = be.put(np.ones((size, D), np.float32)), be.empty((1, D))
    be.check(be.lib.mpqe_scatter_bwd(SCATTER_IDS[op], be.ptr(g), be.ptr(index), be.ptr(arg), 0, D, size, be.ptr(gs),
                                     be.ptr(ws), wsb, be.stream), 'bwd, n_src = 0')
    assert np.isnan(be.get(gs)).all()
    # no segment at all: nothing is written
    src2, index2 = be.put(np.ones((2, D), np.float32)), be.put(np.zeros((2,), np.int64))
    out2 = be.empty((2, D))
    be.check(be.lib.mpqe_scatter_fwd(SCATTER_IDS[op], be.ptr(src2), be.ptr(index2), 2, D, 0, be.ptr(out2), be.ptr(arg),
                                     be.ptr(ws), wsb, be.ptr(err), be.stream), 'dim_size = 0')
    assert np.isnan(be.get(out2)).all()
    assert int(be.get(err)[0]) == 0


@pytest.mark.parametrize('op', ['add', 'max', 'mean'])
def test_scatter_negative_index_is_flagged(be, op):
    """index -1 sets FLAG_BAD_INDEX like an index past the end; that row belongs to no segment (the mean's count does
    not see it, its gradient is zero) and the other rows' results are what they are without it."""
    rng = np.random.RandomState(23)
    n, D, size = 9, 5, 3
    src = rng.randn(n, D).astype(np.float32)
    src[4] = 9.0                                        # would be every column's maximum and move every mean
    index = np.array([0, 1, 2, 0, -1, 1, 2, 0, 1], dtype=np.int64)
    g = rng.randn(size, D).astype(np.float32)
    assert check_scatter(be, op, src, index, size, g) == FLAG_BAD_INDEX
    index[4] = size + 3
    assert check_scatter(be, op, src, index, size, g) == FLAG_BAD_INDEX


# ------------------------------------------------------------------------------------------ cosine
def cosine_ref(q, qrow, t, gs, n_q):
    """include/mpqe_amd.h: s = q.t / (nq nt), nq = max(|q|, eps); csrc/encoder_ops.hip: ds/dq = t/(nq nt) - s q/nq^2, the
    second term only if |q| > eps (and the same for t). Returns s, the per-pair gradients and grad_q summed per query."""
    Q = q.astype(np.float64)[qrow]
    T = t.astype(np.float64)
    rq, rt = np.sqrt((Q * Q).sum(1)), np.sqrt((T * T).sum(1))
    nq, nt = np.maximum(rq, EPS32), np.maximum(rt, EPS32)
    inv = 1.0 / (nq * nt)
    s = (Q * T).sum(1) * inv
    kq = np.where(rq > EPS32, s / (nq * nq), 0.0)
    kt = np.where(rt > EPS32, s / (nt * nt), 0.0)
    g = gs.astype(np.float64)[:, None]
    dq = g * (T * inv[:, None] - kq[:, None] * Q)
    dt = g * (Q * inv[:, None] - kt[:, None] * T)
    grad_q = np.zeros((n_q, q.shape[1]))
    np.add.at(grad_q, qrow, dq)
    return s, dq, dt, grad_q


def run_cosine(be, q, qrow, t, gs, ragged):
    n, D = t.shape
    dq, dt, dr = be.put(q), be.put(t), (be.put(qrow) if ragged else None)
    sc = be.empty((n,))
    be.check(be.lib.mpqe_cosine_fwd(be.ptr(dq), be.ptr(dr), be.ptr(dt), n, D, EPS, be.ptr(sc), be.stream), 'cosine fwd')
    gq = be.zeros(q.shape) if ragged else be.empty(q.shape)      # accumulated into with a row map, overwritten without
    gt = be.empty((n, D))
    dgs = be.put(gs)
    be.check(be.lib.mpqe_cosine_bwd(be.ptr(dgs), be.ptr(dq), be.ptr(dr), be.ptr(dt), n, D, EPS, be.ptr(gq), be.ptr(gt),
                                    be.stream), 'cosine bwd')
    return be.get(sc), be.get(gq), be.get(gt)


def unit_range(rng, shape):
    """magnitudes in [1, 2], random signs. At D = 1 the gradient is the exact cancellation of two terms of size 1/|q|;
    `close`'s floor (2e-6 * max(1, max|ref|)) presumes terms of O(1), which this keeps them at."""
    return (rng.uniform(1.0, 2.0, size=shape) * signs(rng, shape)).astype(np.float32)


@pytest.mark.parametrize('D', [1, 3, 64, 65, 130, 260])
def test_cosine_dense_by_dimension(be, D):
    """one lane, a partial wave, exactly one trip of the per-lane loop, one trip + 1, three trips, past 256; n = 5 is one
    row more than a block owns."""
    rng = np.random.RandomState(100 + D)
    n = 5
    q, t = unit_range(rng, (n, D)), unit_range(rng, (n, D))
    gs = rng.uniform(-1, 1, size=n).astype(np.float32)
    s, dq, dt, _ = cosine_ref(q, np.arange(n), t, gs, n)
    sc, gq, gt = run_cosine(be, q, None, t, gs, ragged=False)
    close(sc, s, what='scores D=%d' % D)
    close(gq, dq, rtol=1e-4, what='grad_q D=%d' % D)
    close(gt, dt, rtol=1e-4, what='grad_t D=%d' % D)


@pytest.mark.parametrize('lengths', [(20, 0, 1), (1,)], ids=['20-0-1', 'n1'])
def test_cosine_ragged(be, lengths):
    """query 0 carries 20 targets (20 atomic adds into one grad_q row, in any order), query 1 none (its grad_q row keeps
    the zeros it arrived with); and n = 1."""
    rng = np.random.RandomState(31)
    B, D = len(lengths), 65
    qrow = np.repeat(np.arange(B), lengths).astype(np.int64)
    n = len(qrow)
    q, t = unit_range(rng, (B, D)), unit_range(rng, (n, D))
    gs = rng.uniform(-1, 1, size=n).astype(np.float32)
    s, dq, dt, grad_q = cosine_ref(q, qrow, t, gs, B)
    sc, gq, gt = run_cosine(be, q, qrow, t, gs, ragged=True)
    close(sc, s, what='scores')
    close(gt, dt, rtol=1e-4, what='grad_t')
    for b in range(B):
        k = lengths[b]
        if k == 0:
            assert (gq[b] == 0).all() and not np.signbit(gq[b]).any()
        elif k == 1:
            close(gq[b], grad_q[b], rtol=1e-4, what='grad_q[%d]' % b)
        else:           # k fp32 additions in any order: k * u * sum|term| per column
            within(gq[b], grad_q[b], k * U * np.abs(dq[qrow == b]).sum(0), 'grad_q[%d] (%d adds)' % (b, k))


@pytest.mark.parametrize('ragged', [False, True], ids=['dense', 'rowmap'])
def test_cosine_degenerate_rows(be, ragged):
    """zero rows, rows below eps (norm 1e-9: clamped, the gradient loses its second term) and just above it (1e-7).
    A clamped or tiny row has gradients of 1e7 .. 1e8, so every row is compared on its own: `close` scales its floor by
    max |ref|, and one such row in a shared comparison would hide any error in the ordinary ones."""
    rng = np.random.RandomState(37)
    D = 6
    names = ['ordinary', 't = 0', 'q = 0', '|q| = 1e-9', '|t| = 1e-9', '|q| = 1e-7', '|t| = 1e-7', 'q = t = 0']
    n = len(names)
    q, t = unit_range(rng, (n, D)), unit_range(rng, (n, D))

    def scaled(v, norm):
        v = v.astype(np.float64)
        return (v / np.sqrt((v * v).sum()) * norm).astype(np.float32)
    t[1] = 0
    q[2] = 0
    q[3] = scaled(q[3], 1e-9)
    t[4] = scaled(t[4], 1e-9)
    q[5] = scaled(q[5], 1e-7)
    t[6] = scaled(t[6], 1e-7)
    q[7] = t[7] = 0
    gs = rng.uniform(0.5, 1, size=n).astype(np.float32)
    s, dq, dt, _ = cosine_ref(q, np.arange(n), t, gs, n)
    # (the cases are what they claim to be: clamped rows have a gradient of about |g| / eps, without the second term)
    assert np.abs(dq[2]).max() > 1e7 and np.abs(dt[1]).max() > 1e7 and np.abs(dq[3]).max() > 1e7
    assert not dq[7].any() and not dt[7].any() and s[1] == 0 and s[2] == 0
    sc, gq, gt = run_cosine(be, q, np.arange(n, dtype=np.int64), t, gs, ragged)
    close(sc, s, what='scores')
    for i, name in enumerate(names):
        close(gq[i], dq[i], rtol=1e-4, what='grad_q, %s' % name)
        close(gt[i], dt[i], rtol=1e-4, what='grad_t, %s' % name)


# ------------------------------------------------------------------------------------------ embedding gather + L2 norm
def embed_problem(D, n, with_map, seed):
    rng = np.random.RandomState(seed)
    rows = 7
    table = rng.randn(rows, D).astype(np.float32)
    if with_map:
        node_map = np.full(12, -1, dtype=np.int64)
        ents = rng.permutation(12)[:rows]
        node_map[ents] = np.arange(rows)
        ids = ents[rng.randint(0, rows, size=n)].astype(np.int64)
    else:
        node_map = None
        ids = rng.randint(0, rows, size=n).astype(np.int64)
    if n > 2:
        ids[2] = ids[0]                                  # a duplicate: two rows of the gradient into one table row
    picked = ids if node_map is None else node_map[ids]
    return table, node_map, ids, picked


@pytest.mark.parametrize('with_map', [True, False], ids=['map', 'identity'])
@pytest.mark.parametrize('n', [1, 5])
@pytest.mark.parametrize('D,stride,offset', [(6, 6, 0), (260, 260, 0), (300, 300, 0), (512, 512, 0), (16, 18, 0),
                                             (16, 16, 1)])
def test_embed_l2norm_fwd_paths(be, D, stride, offset, n, with_map):
    """(6, 6, 0) scalar path; (260 / 300 / 512) a second trip of the 16-byte loop with 1 lane, 11 lanes, every lane; (16,
    18, 0) and (16, 16, 1): a vector-sized row whose stride / whose address rules the vector path out."""
    table, node_map, ids, picked = embed_problem(D, n, with_map, D + n)
    dt, di = be.put(table), be.put(ids)
    dm = None if node_map is None else be.put(node_map)
    tail = 8
    buf = be.empty((4 + n * stride + tail,))
    base = (-(be.ptr(buf) // 4)) % 4 + offset            # floats from the buffer's start to `out`
    assert be.ptr(dt) % 16 == 0 and (be.ptr(buf) + 4 * base) % 16 == 4 * offset
    inv = be.empty((n,))
    err = be.zeros((1,), np.int32)
    be.check(be.lib.mpqe_embed_l2norm_fwd(be.ptr(dt), table.shape[0], D, be.ptr(dm), 0 if node_map is None else len(node_map),
                                          be.ptr(di), n, be.ptr(buf) + 4 * base, stride, be.ptr(inv), be.ptr(err),
                                          be.stream), 'embed fwd')
    v = table.astype(np.float64)[picked]
    nrm = np.sqrt((v * v).sum(1))
    got = be.get(buf)
    written = np.zeros(got.shape, bool)
    for i in range(n):
        written[base + i * stride: base + i * stride + D] = True
    close(got[written].reshape(n, D), v / nrm[:, None], what='y')
    assert np.isnan(got[~written]).all()                 # not between a row's D columns and its stride, not after the last row
    close(be.get(inv), 1.0 / nrm, what='inv_norm')
    assert int(be.get(err)[0]) == 0


@pytest.mark.parametrize('with_map', [True, False], ids=['map', 'identity'])
@pytest.mark.parametrize('D', [6, 260, 300])
def test_embed_l2norm_bwd(be, D, with_map):
    """grad_table[row_i] += (g_i - y_i (y_i . g_i)) / |v_i|, a duplicated id adding twice into one row."""
    n, stride = 5, D + 3
    table, node_map, ids, picked = embed_problem(D, n, with_map, 50 + D)
    assert picked[2] == picked[0]
    rng = np.random.RandomState(D)
    g = rng.randn(n, stride).astype(np.float32)
    v = table.astype(np.float64)[picked]
    nrm = np.sqrt((v * v).sum(1))[:, None]
    y = v / nrm
    g64 = g.astype(np.float64)[:, :D]
    ref = np.zeros(table.shape)
    np.add.at(ref, picked, (g64 - y * (y * g64).sum(1)[:, None]) / nrm)
    dt, di, dg = be.put(table), be.put(ids), be.put(g)
    dm = None if node_map is None else be.put(node_map)
    gt = be.zeros(table.shape)
    err = be.zeros((1,), np.int32)
    be.check(be.lib.mpqe_embed_l2norm_bwd(be.ptr(dg), stride, be.ptr(dt), table.shape[0], D, be.ptr(dm),
                                          0 if node_map is None else len(node_map), be.ptr(di), n, be.ptr(gt), be.ptr(err),
                                          be.stream), 'embed bwd')
    close(be.get(gt), ref, rtol=1e-4, what='grad_table')
    assert int(be.get(err)[0]) == 0


# ------------------------------------------------------------------------------------------ readouts
@pytest.mark.parametrize('kind', ['sum', 'max', 'mp'])
@pytest.mark.parametrize('shape', [(1, 1, 0, 1), (3, 4, 3, 260)], ids=lambda s: 'B%d_N%d_A%d_D%d' % s)
def test_readout_edges(be, kind, shape):
    """N = 1 and D = 1; B * D past one block. Graph 0's rows are all identical (arg 0); graph 1 has {-0.0, +0.0} on top
    of column 0 and {+0.0, -0.0} on top of column 1: equal values, the lowest row wins."""
    B, N, A, D = shape
    rng = np.random.RandomState(B + D)
    h = rng.randn(B, N, D).astype(np.float32)
    if N > 1:
        h[0, 1:] = h[0, 0]
        h[1, :, 0] = [-0.0, 0.0, -1.0, -2.0]
        h[1, :, 1] = [0.0, -0.0, -1.0, -0.0]
    g = rng.randn(B, D).astype(np.float32)
    h64 = h.astype(np.float64)
    out, arg = be.empty((B, D)), be.empty((B, D), np.int32)
    dh, dg = be.put(h.reshape(B * N, D)), be.put(g)
    be.check(be.lib.mpqe_readout_fwd(READOUT_IDS[kind], be.ptr(dh), B, N, A, D, be.ptr(out), be.ptr(arg), be.stream),
             'readout fwd')
    gh = be.empty((B * N, D))
    be.check(be.lib.mpqe_readout_bwd(READOUT_IDS[kind], be.ptr(dg), be.ptr(arg), B, N, A, D, be.ptr(gh), be.stream),
             'readout bwd')
    exp_g = np.zeros((B, N, D))
    if kind == 'sum':
        close(be.get(out), h64.sum(1), what='sum')
        exp_g[:] = g[:, None, :]
    elif kind == 'mp':
        equal(be.get(out), h64[:, A])
        exp_g[:, A] = g
    else:
        best = h64.max(1)
        first = np.argmax(h64 == best[:, None, :], axis=1)
        equal(be.get(out), best)
        equal(be.get(arg), first)
        if N > 1:
            assert (first[0] == 0).all() and first[1, 0] == 0 and first[1, 1] == 0
        for n in range(N):
            exp_g[:, n] = np.where(first == n, g, 0)
    equal(be.get(gh), exp_g.reshape(B * N, D))


# ------------------------------------------------------------------------------------------ variable rows
@pytest.mark.parametrize('B', [1, 70])
def test_var_rows_edges(be, B):
    """D = 130: three column blocks of the backward, the last with 2 columns; B = 1 leaves three of the backward's four
    row groups without a row, B = 70 gives them 18 / 18 / 17 / 17. Mode 3 is used by two variables."""
    rng = np.random.RandomState(40 + B)
    N, A, D, M = 4, 1, 130, 5
    V = N - A
    mode = rng.randn(M, D).astype(np.float32)
    var_ids = np.array([3, 1, 3], dtype=np.int64)
    x = be.empty((B * N, D))
    err = be.zeros((1,), np.int32)
    dm, dv = be.put(mode), be.put(var_ids)
    be.check(be.lib.mpqe_var_rows_fwd(be.ptr(dm), M, D, be.ptr(dv), V, B, N, A, be.ptr(x), be.ptr(err), be.stream), 'fwd')
    xo = be.get(x).reshape(B, N, D)
    assert np.isnan(xo[:, :A]).all()
    equal(xo[:, A:], np.broadcast_to(mode[var_ids][None], (B, V, D)))
    gx = rng.randn(B * N, D).astype(np.float32)
    g0 = rng.randn(M, D).astype(np.float32)
    gm, dgx = be.put(g0), be.put(gx)
    be.check(be.lib.mpqe_var_rows_bwd(be.ptr(dgx), M, D, be.ptr(dv), V, B, N, A, be.ptr(gm), be.ptr(err), be.stream), 'bwd')
    ref = g0.astype(np.float64)
    g3 = gx.reshape(B, N, D).astype(np.float64)
    for k in range(V):
        ref[var_ids[k]] += g3[:, A + k].sum(0)
    got = be.get(gm)
    close(got, ref, what='grad_mode')
    equal(got[[0, 2, 4]], g0[[0, 2, 4]])                  # modes without a variable keep what they held
    assert int(be.get(err)[0]) == 0


# ------------------------------------------------------------------------------------------ hinge
@pytest.mark.parametrize('n', [256, 257])
def test_hinge_at_equality(be, n):
    """loss = mean(clamp(margin - (pos - neg), min = 0)); torch's clamp passes the gradient AT the bound. margin 0.5 and
    terms exactly at equality (0.75 - 0.25), one ulp to either side, clearly clamped and clearly active; n = 257 puts the
    last term on a second trip of the forward's thread 0 and into a second block of the backward."""
    rng = np.random.RandomState(n)
    margin = 0.5
    pos = rng.uniform(-1, 1, size=n).astype(np.float32)
    neg = rng.uniform(-1, 1, size=n).astype(np.float32)
    up, down = np.nextafter(np.float32(0.75), np.float32(1)), np.nextafter(np.float32(0.75), np.float32(0))
    pos[:5], neg[:5] = [0.75, up, down, 2.0, 0.0], [0.25, 0.25, 0.25, 0.0, 1.0]
    pos[n - 1], neg[n - 1] = 0.75, 0.25
    v = margin - (pos.astype(np.float64) - neg.astype(np.float64))
    equal(v[:5], [0.0, -2.0 ** -24, 2.0 ** -24, -1.5, 1.5])       # pos - neg is exact in fp32 for these
    assert v[n - 1] == 0 and (np.abs(v[5:n - 1]) > 1e-6).all()    # the random terms are decided either way
    gl = np.float32(257.0 / 128.0)                                 # gl / 256 and gl / 257 are exact in fp32
    loss = be.empty((1,))
    dp, dn, dgl = be.put(pos), be.put(neg), be.put(np.array([gl], np.float32))
    be.check(be.lib.mpqe_hinge_fwd(be.ptr(dp), be.ptr(dn), n, margin, be.ptr(loss), be.stream), 'hinge fwd')
    close(be.get(loss)[0], np.maximum(v, 0).mean(), what='loss')
    gp, gn = be.empty((n,)), be.empty((n,))
    be.check(be.lib.mpqe_hinge_bwd(be.ptr(dp), be.ptr(dn), n, margin, be.ptr(dgl), be.ptr(gp), be.ptr(gn), be.stream),
             'hinge bwd')
    exp = np.where(v >= 0, float(gl) / n, 0.0)
    assert exp[0] > 0 and exp[1] == 0 and exp[2] > 0 and exp[n - 1] > 0
    equal(be.get(gn), exp)
    equal(be.get(gp), -exp)
    # either output may be left out
    gn2 = be.empty((n,))
    be.check(be.lib.mpqe_hinge_bwd(be.ptr(dp), be.ptr(dn), n, margin, be.ptr(dgl), None, be.ptr(gn2), be.stream), 'no grad_pos')
    equal(be.get(gn2), exp)


# ------------------------------------------------------------------------------------------ LayerNorm + ReLU
LN_EPS = 1e-6
_LN = {}


def layernorm_problem(rows, D, relu):
    """Inputs and the float64 autograd of  y = act(gamma (x - mean) / (std + eps) + beta),  std unbiased. Computed once per
    case and shared by the backends. The first seed is taken for which the float64 values alone show (a) no pre-activation
    within 1e-5 of 0 (there the ReLU's mask is a coin toss in fp32) and (b) no row with std < 1: grad_x is a difference of
    terms of size |g gamma| / std (at D = 2 they cancel to nothing), and `close`'s floor presumes terms of O(1)."""
    key = (rows, D, relu)
    if key in _LN:
        return _LN[key]
    for seed in range(1000):
        rng = np.random.RandomState(1000 * D + 10 * rows + seed)
        x = (rng.randn(rows, D) * 2 + 0.3).astype(np.float32)
        gamma, beta = (rng.rand(D) + 0.5).astype(np.float32), (rng.randn(D) * 0.3).astype(np.float32)
        gy = rng.randn(rows, D).astype(np.float32)
        xt, gt, bt = [torch.from_numpy(a.astype(np.float64)).requires_grad_(True) for a in (x, gamma, beta)]
        std = xt.std(-1, keepdim=True)
        pre = gt * (xt - xt.mean(-1, keepdim=True)) / (std + float(np.float32(LN_EPS))) + bt
        if float(std.detach().min()) < 1.0 or (relu and float(pre.detach().abs().min()) < 1e-5):
            continue
        y = torch.relu(pre) if relu else pre
        y.backward(torch.from_numpy(gy.astype(np.float64)))
        _LN[key] = (x, gamma, beta, gy, y.detach().numpy(), xt.grad.numpy(), gt.grad.numpy(), bt.grad.numpy(),
                    xt.detach().mean(-1).numpy(), (1.0 / (std + float(np.float32(LN_EPS)))).detach().numpy()[:, 0])
        return _LN[key]
    raise AssertionError('no settled LayerNorm problem')


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('rows', [1, 5, 9])
@pytest.mark.parametrize('D', [2, 65, 260, 300])
def test_layernorm_relu_edges(be, D, rows, relu):
    """D = 2 (the smallest with a std), 65 (one trip + 1 lane), 260 and 300 (five trips, 4 and 44 lanes on the last);
    rows 1 / 5 / 9: block tails at 4 rows per block."""
    check_layernorm(be, D, rows, relu)


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('D', [64, 65])
def test_layernorm_relu_column_sums_past_128_partial_rows(be, D, relu):
    """grad_gamma and grad_beta are column sums through csrc/bias_grad.h. rows = 4097: 129 partial rows, so
    bias_final_kernel makes a second trip with one row on it; D = 64 takes the 16-byte partial sums (16 row groups per
    trip, the clamped rows past each block's 32 left out), D = 65 the scalar ones with a second column block of one column."""
    from tests.test_dense_template_edges import bias_form, bias_num_blocks
    rows = 4097
    assert bias_num_blocks(rows) == 129 and bias_form(D) == {64: ('v4', 16), 65: ('scalar', 0)}[D]
    check_layernorm(be, D, rows, relu)


def check_layernorm(be, D, rows, relu):
    x, gamma, beta, gy, y_ref, gx_ref, gg_ref, gb_ref, mean_ref, inv_ref = layernorm_problem(rows, D, relu)
    dx, dg, db, dgy = be.put(x), be.put(gamma), be.put(beta), be.put(gy)
    y, stats = be.empty((rows, D)), be.empty((rows, 2))
    be.check(be.lib.mpqe_layernorm_relu_fwd(be.ptr(dx), rows, D, be.ptr(dg), be.ptr(db), LN_EPS, relu, be.ptr(y),
                                            be.ptr(stats), be.stream), 'ln fwd')
    close(be.get(y), y_ref, what='y')
    st = be.get(stats)
    close(st[:, 0], mean_ref, what='stats: mean')
    close(st[:, 1], inv_ref, what='stats: 1 / (std + eps)')
    gx, gg, gb = be.empty((rows, D)), be.zeros((D,)), be.zeros((D,))
    wb = be.lib.mpqe_layernorm_relu_bwd_workspace_bytes(rows, D)
    ws = be.nbytes(wb + 256)
    be.check(be.lib.mpqe_layernorm_relu_bwd(be.ptr(dgy), be.ptr(dx), be.ptr(y), rows, D, be.ptr(dg), be.ptr(stats), LN_EPS,
                                            relu, be.ptr(gx), be.ptr(gg), be.ptr(gb), (be.ptr(ws) + 255) // 256 * 256, wb,
                                            be.stream), 'ln bwd')
    close(be.get(gx), gx_ref, rtol=1e-4, what='grad_x')
    close(be.get(gg), gg_ref, rtol=1e-4, what='grad_gamma')
    close(be.get(gb), gb_ref, rtol=1e-4, what='grad_beta')


# ------------------------------------------------------------------------------------------ branch aggregate
@pytest.mark.parametrize('count', [1, 256, 257, 1000])
@pytest.mark.parametrize('agg', ['mean', 'min'])
@pytest.mark.parametrize('branches', [2, 3])
def test_branch_agg(be, branches, agg, count):
    """out = mean / min of two or three arrays, element by element; the minimum's gradient goes to the FIRST branch that
    holds it, the others get exact zeros. Small integers as values: a large share of the elements are exact ties."""
    rng = np.random.RandomState(7 * count + branches)
    xs = [rng.randint(-2, 3, size=count).astype(np.float32) for _ in range(branches)]
    g = rng.randn(count).astype(np.float32)
    X = np.stack(xs).astype(np.float64)
    if count >= 256:
        assert ((X == X.min(0)).sum(0) > 1).mean() > 0.1         # ties are common
    d = [be.put(a) for a in xs] + [None] * (3 - branches)
    dg = be.put(g)
    out = be.empty((count,))
    code = int(agg == 'min')
    be.check(be.lib.mpqe_branch_agg_fwd(be.ptr(d[0]), be.ptr(d[1]), be.ptr(d[2]), count, code, be.ptr(out), be.stream), 'fwd')
    gs = [be.empty((count,)) for _ in range(3)]            # with two branches grad_x2 has nothing to receive
    be.check(be.lib.mpqe_branch_agg_bwd(be.ptr(d[0]), be.ptr(d[1]), be.ptr(d[2]), count, code, be.ptr(dg), be.ptr(gs[0]),
                                        be.ptr(gs[1]), be.ptr(gs[2]), be.stream), 'bwd')
    if agg == 'min':
        equal(be.get(out), X.min(0))
        first = np.argmax(X == X.min(0), axis=0)
        exp = [np.where(first == k, g, 0.0) for k in range(branches)]
    else:
        got, ref = report(be.get(out), X.mean(0), 'mean')
        np.testing.assert_allclose(got, ref, rtol=1e-6, atol=0)     # the sum of small integers is exact: one rounding, of the / 3
        exp = [g.astype(np.float64) / branches] * branches
    for k in range(branches):
        if agg == 'min':
            equal(be.get(gs[k]), exp[k], 'grad_x%d' % k)
        else:
            got, ref = report(be.get(gs[k]), exp[k], 'grad_x%d' % k)
            np.testing.assert_allclose(got, ref, rtol=1e-6, atol=0)
    if branches == 2:
        assert np.isnan(be.get(gs[2])).all()
    # outputs passed as NULL are skipped, the others are still right
    g1, g2 = be.empty((count,)), be.empty((count,))
    be.check(be.lib.mpqe_branch_agg_bwd(be.ptr(d[0]), be.ptr(d[1]), be.ptr(d[2]), count, code, be.ptr(dg), None, be.ptr(g1),
                                        be.ptr(g2) if branches == 3 else None, be.stream), 'bwd, grad_x0 = NULL')
    equal(be.get(g1), be.get(gs[1]))
    if branches == 3:
        equal(be.get(g2), be.get(gs[2]))


# ------------------------------------------------------------------------------------------ optimiser steps
def optim_grid(n, per_thread):
    """csrc/optim.hip: workgroups of 256 threads, `per_thread` elements each, at most 4096 of them"""
    return max(min(-(-n // (256 * per_thread)), 256 * 16), 1)


def at_offset(be, a, off):
    """`a` on the backend, starting 4 * off bytes past a 16-byte boundary"""
    buf = be.zeros((a.size + 8,))
    base = (-(be.ptr(buf) // 4)) % 4 + off
    view = buf[base:base + a.size]
    if be.name == 'emu':
        view[:] = a
    else:
        view.copy_(be.torch.from_numpy(a))
    assert be.ptr(view) % 16 == 4 * off
    return view


def check_adam(be, n, wd, steps, offs, edges):
    """mpqe_adam_step against torch.optim.Adam on the CPU with tests/test_kernels.py::test_adam_step_matches_torch's
    tolerances (they come from the reference's arithmetic: a few ulps of p ~ 1, one rounding of an O(3) intermediate); the
    elements at `edges` are compared one by one on top of the whole arrays. offs: floats past a 16-byte boundary of
    (param, grad, exp_avg, exp_avg_sq)."""
    rng = np.random.RandomState(n % 1000 + sum(offs))
    p0 = rng.randn(n).astype(np.float32)
    ref = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([ref], lr=0.01, weight_decay=wd)
    zeros = np.zeros(n, np.float32)
    p, m, v = at_offset(be, p0, offs[0]), at_offset(be, zeros, offs[2]), at_offset(be, zeros, offs[3])
    for t in range(1, steps + 1):
        g = (rng.randn(n) * (0.1 if t % 2 else 3.0)).astype(np.float32)
        ref.grad = torch.from_numpy(g.copy())
        opt.step()
        dg = at_offset(be, g, offs[1])
        be.check(be.lib.mpqe_adam_step(be.ptr(p), be.ptr(dg), be.ptr(m), be.ptr(v), n, 0.01, 0.9, 0.999, 1e-8, wd, t,
                                       be.stream), 'adam')
    state = opt.state[ref]
    for got, want, rtol, atol, what in ((p, ref.detach(), 2e-6, 3e-7, 'param'), (m, state['exp_avg'], 1e-6, 3e-7, 'exp_avg'),
                                        (v, state['exp_avg_sq'], 2e-6, 1e-9, 'exp_avg_sq')):
        got, want = be.get(got), want.numpy()
        for i in edges:
            np.testing.assert_allclose(got[i], want[i], rtol=rtol, atol=atol, err_msg='%s[%d]' % (what, i))
        np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg=what)
    moved = be.get(p)[list(edges)] != p0[list(edges)]
    assert moved.all()


def test_adam_step_second_grid_stride_trip(be):
    """n = 4 194 304 + 5: the grid is capped at 4096 workgroups of 1024 elements, so thread 0 makes a second trip with a
    whole vector on it (elements n - 5 .. n - 2) and thread 1 one whose `i + 3 < n` fails: the scalar tail (element n - 1).
    Two steps. The emulator takes 2 s: it runs there too.
    No weight decay here (the scalar-path cases have it): among four million elements some g + wd p cancels down to the
    size of eps = 1e-8, where the first step's m / (sqrt(v) + eps) magnifies the rounding of that sum a thousandfold. With
    wd = 1e-3 one element did (g = -5.979811e-4, p = 0.59799045): torch's float32 result lay 7.6e-6 from the float64 one and
    the kernel's 3.7e-6, which says nothing about either. Without weight decay the sum is g itself, exactly."""
    n, first = 4194304 + 5, 4096 * 1024
    assert optim_grid(n, 4) == 4096 and -(-n // 4) == 4096 * 256 + 2          # two threads' worth beyond the first trip
    check_adam(be, n, 0.0, 2, (0, 0, 0, 0), edges=(0, first - 4, first - 1, first, first + 3, first + 4))


ADAM_OFFSETS = {'all': (1, 1, 1, 1), 'param': (1, 0, 0, 0), 'grad': (0, 1, 0, 0), 'exp_avg': (0, 0, 1, 0),
                'exp_avg_sq': (0, 0, 0, 1)}


@pytest.mark.parametrize('which', list(ADAM_OFFSETS))
def test_adam_step_scalar_path(be, which):
    """n = 4099 with all four buffers 4 bytes past a 16-byte boundary, then each alone: every term of the host's `vec`
    sends the call to the scalar loop, whose 5 workgroups (the grid is sized for four elements a thread) make four trips,
    the last of 259 elements."""
    n = 4099
    stride = optim_grid(n, 4) * 256
    assert stride == 1280 and -(-n // stride) == 4 and n - 3 * stride == 259
    check_adam(be, n, 1e-3, 3, ADAM_OFFSETS[which], edges=(0, stride - 1, stride, 3 * stride - 1, 3 * stride, n - 1))


def test_sgd_step_second_grid_stride_trip(be):
    """n = 1 048 576 + 3: sgd_kernel's grid is capped at 4096 workgroups of 256 elements, so threads 0 .. 2 make a second
    trip. Tolerance of tests/test_kernels.py::test_sgd_step_matches_torch. The emulator takes under 1 s: it runs there too."""
    n, first = 1048576 + 3, 4096 * 256
    assert optim_grid(n, 1) == 4096 and n - first == 3
    rng = np.random.RandomState(11)
    p0, g = rng.randn(n).astype(np.float32), rng.randn(n).astype(np.float32)
    ref = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    ref.grad = torch.from_numpy(g.copy())
    torch.optim.SGD([ref], lr=0.05, momentum=0, weight_decay=1e-2).step()
    p, dg = be.put(p0), be.put(g)
    be.check(be.lib.mpqe_sgd_step(be.ptr(p), be.ptr(dg), n, 0.05, 1e-2, be.stream), 'sgd')
    got, want = be.get(p), ref.detach().numpy()
    for i in (0, first - 1, first, first + 1, n - 1):
        np.testing.assert_allclose(got[i], want[i], rtol=1e-6, atol=1e-7, err_msg='param[%d]' % i)
        assert got[i] != p0[i]
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-7)
