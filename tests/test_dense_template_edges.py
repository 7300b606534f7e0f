"""The dense layer (csrc/dense.hip), the template R-GCN layer (csrc/rgcn_template.hip) and the bias-gradient reduction they
share (csrc/bias_grad.h) exactly at the edges of their K-split planners: chunk counts of 1, 2, 8, 9, 17, 64 and the capped
regimes beyond, one-row last chunks, more than 128 and exactly 1024 partial bias rows, every width form of the bias sums.

The method is tests/test_general_edges.py's. Every operand -- x, weights, bias, the upstream gradient, what accumulate-mode
outputs start with -- is a small integer stored as float32 (uniform in {-2 .. 2}) and the oracle is the same operation in
numpy int64: ReLU as `pre > 0`, the gradients behind the mask `out > 0`. Each case first asserts from its own data that the
oracle run on the ABSOLUTE values, nothing masked away and the accumulate contents included, stays below 2^24: then every
float32 product and partial sum is an integer that float32 holds, in whatever order a kernel adds them, and every comparison
below is an equality. One dropped or doubled chunk, slab, K-step or partial row shows; no tolerance that float32 sums of
Gaussian data over thousands of rows need would let it. The backward's mask operand is the ORACLE's output, so a forward
fault cannot hide a backward one. Workspaces arrive filled with NaN: a slab or partial row that is read without having been
written shows as well.

The planners are restated here in Python (dense_chunks, plan_chunks, bias_rows_per_block, the load-mode conditions); each
case asserts the regime it was chosen for from those copies, and pins the copies to the library through the workspace sizes
the library reports, which are functions of the chunk and partial-row counts.

Runs on the host emulator (`emu`) and on the gfx950 library (`hip`, marked gpu), tests/test_kernels.py's fixture pattern.
The cases that run on `hip` alone, because the emulator needs more than about ten seconds for them, are named at
HIP_ONLY_DENSE with the emulator's measured times; each regime they cover keeps `emu` cases at smaller dims.
"""
import numpy as np
import pytest

from mpqe_amd._capi import QUERY_TYPE_IDS
from oracle import ref_cpu

GT_BM, GT_BN, GT_BK = 64, 64, 32        # csrc/gemm_core.h
DIMS = [(64, 64), (40, 24), (5, 3)]     # LD_FAST / LD_PRED / LD_SCALAR when every pointer is 16-byte aligned
dims_id = lambda d: '%dx%d' % d
FAST, PRED, SCALAR = 'LD_FAST', 'LD_PRED', 'LD_SCALAR'


@pytest.fixture(scope='module', params=['emu', pytest.param('hip', marks=pytest.mark.gpu)])
def be(request):
    from tests import kernel_backend
    if request.param == 'emu':
        return kernel_backend.EmuBackend()
    return kernel_backend.HipBackend()


# ------------------------------------------------------------------------------------------ the planners, restated
def ceil_div(a, b):
    return -(-a // b)


def align_up(v, a):
    return ceil_div(v, a) * a


def _pick(count, per_chunk, max_chunks):
    """the rule dense_chunks and plan_chunks share: -> (chunks, rows of a chunk: a multiple of the K-step)"""
    n = min(max(ceil_div(count, per_chunk), 1), max_chunks)
    c = max(align_up(ceil_div(count, n), GT_BK), GT_BK)
    return max(ceil_div(count, c), 1), c


def dense_chunks(rows):
    """csrc/dense.hip: dense_chunks -> (nch, ch)"""
    return _pick(rows, 256, 64)


def plan_chunks(B, N):
    """csrc/rgcn_template.hip: plan_chunks -> ((nch_edge, ch_edge), (nch_root, ch_root))"""
    return _pick(B, 128, 16), _pick(B * N, 128, 32)


def last_chunk(count, plan):
    nch, ch = plan
    return count - (nch - 1) * ch


def bias_rows_per_block(rows):
    """csrc/bias_grad.h"""
    return max(ceil_div(rows, 1024), 32)


def bias_num_blocks(rows):
    return ceil_div(rows, bias_rows_per_block(rows))


def bias_form(dout):
    """launch_bias_grad's choice when its pointers are 16-byte aligned: ('v4', row groups of a trip) or ('scalar', 0)"""
    if dout % 64 == 0 and dout <= 1024 and 256 % (dout // 4) == 0:
        return 'v4', 256 // (dout // 4)
    return 'scalar', 0


def bias_partial_bytes(rows, dout):
    return align_up(bias_num_blocks(rows) * dout * 4, 256)


def gemm_mode(vec, k, n):
    """the host's three-way switch of a tile-core launch: K extent `k` in whole K-steps, output columns `n` in whole tiles"""
    return FAST if vec and k % GT_BK == 0 and n % GT_BN == 0 else PRED if vec else SCALAR


def dense_modes(rows, din, dout, ld):
    """mpqe_linear_fwd / mpqe_linear_bwd with every pointer 16-byte aligned -> modes of (forward, grad_x, grad_W)"""
    vec_f = din % 4 == 0 and ld % 4 == 0
    vec_b = vec_f and dout % 4 == 0
    return (gemm_mode(vec_f, din, dout), gemm_mode(vec_b, dout, din),
            FAST if vec_b and din % GT_BM == 0 and dout % GT_BN == 0 and rows % GT_BK == 0 else PRED if vec_b else SCALAR)


def tmpl_grad_w_mode(B, din, dout):
    vec = dout % 4 == 0 and din % 4 == 0 and (din * dout) % 4 == 0
    return FAST if vec and din % GT_BM == 0 and dout % GT_BN == 0 and B % GT_BK == 0 else PRED if vec else SCALAR


# ------------------------------------------------------------------------------------------ data
def small_ints(rng, shape):
    return rng.randint(-2, 3, size=shape, dtype=np.int8).astype(np.float32)


def i64(a):
    return a.astype(np.int64)


def same(got, want, what):
    np.testing.assert_array_equal(got, want, err_msg=what)


_cases = {}


def cached(key, make):
    """cases are built, and their oracles computed, once for both backends"""
    if key not in _cases:
        _cases[key] = make()
    return _cases[key]


def nan_workspace(be, nbytes):
    """the library's workspace, 16-byte aligned and filled with NaN: what was not written must not be read"""
    ws = be.nbytes(nbytes)
    (ws.fill if be.name == 'emu' else ws.fill_)(float('nan'))
    assert be.ptr(ws) % 16 == 0
    return ws


def aligned(be, *arrays):
    return all(a is None or be.ptr(a) % 16 == 0 for a in arrays)


# ------------------------------------------------------------------------------------------ dense layer: oracle, driver
FENCE = np.float32(-77.0)               # what the columns of grad_W's matrix outside the block hold


class DenseCase(object):
    """y = [relu](x . W^T + bias) on the column block [off, off + din) of a [dout, din + pad] matrix, the upstream gradient
    and what the accumulate-mode outputs start with."""

    def __init__(self, rows, dims, seed, pad=0, off=0, bias_only=False):
        rng = np.random.RandomState(seed)
        self.rows, (self.din, self.dout), self.ld, self.off = rows, dims, dims[0] + pad, off
        din, dout = dims
        self.x, self.W, self.bias = small_ints(rng, (rows, din)), small_ints(rng, (dout, din)), small_ints(rng, (dout,))
        self.g = small_ints(rng, (rows, dout))
        self.bias_only = bias_only              # only grad_bias will be asked for: no y0, no oracle of the other gradients
        self.y0 = None if bias_only else small_ints(rng, (rows, dout))
        self.gW0, self.gb0 = small_ints(rng, (dout, din)), small_ints(rng, (dout,))
        self._ref = {}

    def reference(self, relu):
        if relu not in self._ref:
            ops = [self.x, self.W, self.bias, self.g, self.y0, self.gW0, self.gb0]
            ref = _dense_int64(*[None if a is None else i64(a) for a in ops], relu=relu, bias_only=self.bias_only)
            # the same sums over absolute values, no term masked away: an upper bound of every partial sum in every order
            bound = _dense_int64(*[None if a is None else np.abs(i64(a)) for a in ops], relu=0, bias_only=self.bias_only)
            ref['bound'] = max(int(bound[k].max()) for k in ('y', 'y_acc', 'x', 'W_acc', 'bias_acc') if k in bound)
            self._ref[relu] = ref
        return self._ref[relu]


def _dense_int64(x, W, bias, g, y0, gW0, gb0, relu, bias_only=False):
    pre = x @ W.T + bias
    act = (lambda p: np.where(p > 0, p, 0)) if relu else (lambda p: p)
    gpre = np.where(pre > 0, g, 0) if relu else g
    gb = gpre.sum(0)
    ref = dict(y=act(pre), bias=gb, bias_acc=gb + gb0)
    if not bias_only:
        gW = gpre.T @ x
        ref.update(y_acc=act(pre + y0), x=gpre @ W, W=gW, W_acc=gW + gW0)
    return ref


def in_block(c, a, fill):
    """`a` [dout, din] as the column block of a [dout, ld] matrix whose other columns hold `fill`"""
    full = np.full((c.dout, c.ld), fill, dtype=np.float32)
    full[:, c.off:c.off + c.din] = a
    return full


def dense_forward(be, c, relu, accumulate):
    x, bias = be.put(c.x), be.put(c.bias)
    Wm = be.put(in_block(c, c.W, np.nan))           # reads must stay inside W[0:dout, 0:din] of the block
    W = Wm[:, c.off:c.off + c.din]
    y = be.put(c.y0) if accumulate else be.empty((c.rows, c.dout))
    be.check(be.lib.mpqe_linear_fwd(be.ptr(x), c.rows, be.ptr(W), c.ld, be.ptr(bias), c.din, c.dout, relu, accumulate,
                                    be.ptr(y), be.stream), 'linear fwd (accumulate %d)' % accumulate)
    return be.get(y), aligned(be, x, W)


def dense_backward(be, c, relu, overwrite, want=('x', 'W', 'bias')):
    """-> ({name: array}, the whole [dout, ld] matrix that holds grad_W's block, whether every pointer was 16-byte
    aligned). Outputs not in `want` go in as NULL. Overwrite mode writes onto NaN, accumulate mode onto the case's integer
    contents (grad_x is written whole in both)."""
    ref = c.reference(relu)
    x, g = be.put(c.x), be.put(c.g)
    Wm = be.put(in_block(c, c.W, np.nan))
    W = Wm[:, c.off:c.off + c.din]
    y = be.put(ref['y'].astype(np.float32)) if relu else None       # the oracle's output is the mask
    gx = be.empty((c.rows, c.din)) if 'x' in want else None
    gWm = gW = gb = None
    if 'W' in want:
        gWm = be.put(in_block(c, np.full((c.dout, c.din), np.nan, np.float32) if overwrite else c.gW0, FENCE))
        gW = gWm[:, c.off:c.off + c.din]
    if 'bias' in want:
        gb = be.empty((c.dout,)) if overwrite else be.put(c.gb0)
    wb = be.lib.mpqe_linear_bwd_workspace_bytes(c.rows, c.din, c.dout)
    nch, _ = dense_chunks(c.rows)
    assert wb == align_up(nch * c.din * c.dout * 4, 256) + bias_partial_bytes(c.rows, c.dout) + 256     # the copies hold
    ws = nan_workspace(be, wb)
    be.check(be.lib.mpqe_linear_bwd(be.ptr(x), c.rows, be.ptr(W), c.ld, be.ptr(y), be.ptr(g), c.din, c.dout, relu, overwrite,
                                    be.ptr(gx), be.ptr(gW), c.ld, be.ptr(gb), be.ptr(ws), wb, be.stream),
             'linear bwd (%s)' % ('overwrite' if overwrite else 'accumulate'))
    got = {k: be.get(b) for k, b in (('x', gx), ('W', gW), ('bias', gb)) if b is not None}
    return got, None if gWm is None else be.get(gWm), aligned(be, x, W, y, g, ws)


def check_dense(be, c, relu, forward=True, want=('x', 'W', 'bias')):
    """forward in overwrite and accumulate mode, backward in overwrite and accumulate mode -> whether every pointer of the
    backward was 16-byte aligned (what the load-mode assertions of the callers presume)"""
    ref = c.reference(relu)
    assert ref['bound'] < 2 ** 24           # every sum below is exact in float32, in any order
    if forward:
        for accumulate in (0, 1):
            y, _ = dense_forward(be, c, relu, accumulate)
            same(y, ref['y_acc' if accumulate else 'y'], 'y (accumulate %d)' % accumulate)
    for overwrite in (1, 0):
        got, gWm, al = dense_backward(be, c, relu, overwrite, want)
        assert set(got) == set(want)
        mode = 'overwrite' if overwrite else 'accumulate'
        if 'x' in want:
            same(got['x'], ref['x'], 'grad_x (%s)' % mode)
        if 'W' in want:
            same(got['W'], ref['W' if overwrite else 'W_acc'], 'grad_W (%s)' % mode)
            outside = np.ones((c.dout, c.ld), bool)
            outside[:, c.off:c.off + c.din] = False
            same(gWm[outside].view(np.int32), np.full(int(outside.sum()), FENCE).view(np.int32),
                 'columns of grad_W outside the block (%s)' % mode)
        if 'bias' in want:
            same(got['bias'], ref['bias' if overwrite else 'bias_acc'], 'grad_bias (%s)' % mode)
    return al


# ------------------------------------------------------------------------------------------ A: dense, chunk regimes
#             rows: (nch, rows of a chunk, rows of the last chunk)
DENSE_ROWS = {33: (1, 64, 33),
              257: (2, 160, 97),            # the reduction adds two slabs; dense_grad_w_kernel with blockIdx.x = 1
              288: (2, 160, 128),
              2048: (8, 256, 256),          # exactly one unrolled trip of the reduction, no remainder
              2049: (9, 256, 1),            # a one-row last chunk; 8 + 1 in the reduction
              4097: (17, 256, 1),           # two unrolled trips + 1; 129 partial bias rows: a second trip of bias_final_kernel
              16384: (64, 256, 256),        # the most chunks there are, at the uncapped chunk length
              16385: (57, 288, 257),        # the 64-chunk cap: chunks longer than 256 rows
              32769: (61, 544, 129),        # bias rows per block 33, 993 partial rows
              33792: (63, 544, 64)}         # 1024 partial bias rows: the most there are
# On `hip` alone: 32769 and 33792 rows at 64 x 64, for which the emulator needs 12 s a case (it needs 6 s at 16384 and
# 16385 rows, which stay). The same rows run on `emu` at 40 x 24 (8 s) and 5 x 3 (6 s); the LD_FAST weight gradient runs
# there at up to 64 chunks (16384 rows), its one case under the cap (33792) does not.
HIP_ONLY_DENSE = {(r, (64, 64)) for r in (32769, 33792)}


def dense_case(rows, dims, pad=0, off=0):
    return cached(('dense', rows, dims, pad, off), lambda: DenseCase(rows, dims, seed=100 + rows % 97 + dims[0], pad=pad, off=off))


@pytest.fixture(scope='module', params=[pytest.param('hip', marks=pytest.mark.gpu)])
def hip(request):
    from tests import kernel_backend
    return kernel_backend.HipBackend()


DENSE_CASES = [(r, d) for r in sorted(DENSE_ROWS) for d in DIMS]
case_id = lambda v: dims_id(v) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('rows,dims', [c for c in DENSE_CASES if c not in HIP_ONLY_DENSE], ids=case_id)
def test_dense_chunk_regimes(be, rows, dims, relu):
    """mpqe_linear_fwd (overwrite, accumulate) and mpqe_linear_bwd (overwrite, accumulate) at every chunk count of
    dense_chunks that takes dense_reduce_w_kernel through another path, and at the partial-row counts of the bias sums.
    Emulator time of the slowest cases that run there (32769 and 33792 rows at 40 x 24): 8 s."""
    dense_chunk_regime(be, rows, dims, relu)


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('rows,dims', sorted(HIP_ONLY_DENSE), ids=case_id)
def test_dense_chunk_regimes_on_hip_alone(hip, rows, dims, relu):
    """The two largest row counts at 64 x 64 (HIP_ONLY_DENSE): the same checks, on the gfx950 library only."""
    dense_chunk_regime(hip, rows, dims, relu)


def dense_chunk_regime(be, rows, dims, relu):
    nch, ch = dense_chunks(rows)
    assert (nch, ch, last_chunk(rows, (nch, ch))) == DENSE_ROWS[rows]
    assert (nch > 1) == (rows > 256) and (ch > 256) == (rows > 16384) and ch % GT_BK == 0
    # the reduction: whole unrolled trips of 8 slabs, then the remainder loop
    assert (nch // 8, nch % 8) == {1: (0, 1), 2: (0, 2), 8: (1, 0), 9: (1, 1), 17: (2, 1), 64: (8, 0), 57: (7, 1),
                                   61: (7, 5), 63: (7, 7)}[nch]
    # the bias sums: partial rows, and the trips of bias_final_kernel over them (128 a trip)
    rpb, nblk = bias_rows_per_block(rows), bias_num_blocks(rows)
    assert (rpb > 32) == (rows > 32768) and (nblk > 128) == (rows > 4096)
    if rows in (4097, 32769, 33792):
        assert (rpb, nblk) == {4097: (32, 129), 32769: (33, 993), 33792: (33, 1024)}[rows]
    c = dense_case(rows, dims)
    al = check_dense(be, c, relu)
    # which loads ran: the weight gradient's K dimension is the rows, so its LD_FAST asks for rows % 32 == 0
    assert al
    fwd, bwd_x, grad_w = dense_modes(rows, c.din, c.dout, c.ld)
    if dims == (64, 64):
        assert fwd == bwd_x == FAST
        assert (grad_w == FAST) == (rows in (288, 2048, 16384, 33792)) and grad_w in (FAST, PRED)
    else:
        assert fwd == bwd_x == grad_w == (PRED if dims == (40, 24) else SCALAR)


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('dims', DIMS, ids=dims_id)
@pytest.mark.parametrize('rows', [257, 2049])
def test_dense_column_block_of_a_wider_matrix(be, rows, dims, relu):
    """ldw = ldgw = din + 8 with the block 4 columns in (the encoder's compress blocks): W's other columns are NaN, those
    of grad_W's matrix hold a fence value that must come back bit for bit, through two and through nine chunks."""
    c = dense_case(rows, dims, pad=8, off=4)
    assert c.ld > c.din and dense_chunks(rows)[0] in (2, 9)
    assert check_dense(be, c, relu)
    assert dense_modes(rows, c.din, c.dout, c.ld)[2] == {(64, 64): PRED, (40, 24): PRED, (5, 3): SCALAR}[dims]


# ------------------------------------------------------------------------------------------ B: dense, bias forms
#             dout: (form, row groups of a trip of bias_partial4_kernel)
BIAS_DOUTS = {64: ('v4', 16), 256: ('v4', 4), 512: ('v4', 2), 1024: ('v4', 1),
              192: ('scalar', 0), 320: ('scalar', 0),           # multiples of 64, but 256 % (dout / 4) != 0
              65: ('scalar', 0)}


_bias_case = [None, None]


def bias_case(rows, dout):
    """(kept for the next value of relu only, not for the other backend: 134 MB per operand at dout = 1024)"""
    if _bias_case[0] != (rows, dout):
        _bias_case[:] = [(rows, dout), DenseCase(rows, (4, dout), seed=200 + rows % 89 + dout, bias_only=True)]
    return _bias_case[1]


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('dout', sorted(BIAS_DOUTS))
@pytest.mark.parametrize('rows', [33, 4097, 32769])
def test_dense_bias_forms(be, rows, dout, relu):
    """grad_bias through every width form of the partial sums: the 16-byte form with 16, 4, 2 and 1 row groups per trip --
    the last block's rows never fill its 8 trips in flight, so the clamped rows past its end are loaded and must stay out
    of the sums --, and the scalar form at 192, 320 (multiples of 64 that the 16-byte form cannot split a workgroup over)
    and 65. Rows: two partial rows, the second of one row; 129 partial rows; 33 rows per block and 993 partial rows. Only the backward runs, in overwrite and in accumulate mode, with grad_bias its only
    output: grad_W over din = 4 would cost the emulator 22 s at 32769 x 1024 and is the chunk-regime cases' matter. Every
    case runs on both backends; the emulator's slowest (32769 rows, dout 1024) takes 3 s, most of it the int64 oracle."""
    form, rg = bias_form(dout)
    assert (form, rg) == BIAS_DOUTS[dout]
    rpb, nblk = bias_rows_per_block(rows), bias_num_blocks(rows)
    assert (rpb, nblk, rows - (nblk - 1) * rpb) == {33: (32, 2, 1), 4097: (32, 129, 1), 32769: (33, 993, 33)}[rows]
    if form == 'v4':        # 8 * rg rows are in flight per trip: the last block's rows never fill its last trip
        assert (rows - (nblk - 1) * rpb) % (8 * rg) != 0
    c = bias_case(rows, dout)
    assert check_dense(be, c, relu, forward=False, want=('bias',))


# ------------------------------------------------------------------------------------------ template layer: oracle, driver
OUTPUTS = ('x', 'basis', 'root', 'bias')
R = 4                                   # relations of the basis stack; at least one never belongs to a template edge


class TmplCase(object):
    """B replicas of one query template (row = b * N + n), its operands, the upstream gradient and what the gradient
    outputs hold before the call (the template backward always accumulates; grad_x is written whole)."""

    def __init__(self, qt, rels, B, dims, seed):
        rng = np.random.RandomState(seed)
        t = ref_cpu.TEMPLATES[qt]
        self.qt, self.B, (self.Din, self.Dout) = qt, B, dims
        self.src, self.dst, self.rels = list(t['src']), list(t['dst']), list(rels)
        self.N, self.E = 1 + max(self.src + self.dst), len(self.src)
        assert len(self.rels) == self.E
        Din, Dout = dims
        self.x, self.basis, self.root = small_ints(rng, (B * self.N, Din)), small_ints(rng, (R, Din, Dout)), small_ints(rng, (Din, Dout))
        self.bias, self.gout = small_ints(rng, (Dout,)), small_ints(rng, (B * self.N, Dout))
        self.init = dict(basis=small_ints(rng, (R, Din, Dout)), root=small_ints(rng, (Din, Dout)), bias=small_ints(rng, (Dout,)))
        self._ref = {}

    def reference(self, relu):
        if relu not in self._ref:
            ops = [i64(a) for a in (self.x, self.basis, self.root, self.bias, self.gout)]
            ref = _tmpl_int64(self, *ops, relu=relu)
            bound = _tmpl_int64(self, *[np.abs(a) for a in ops], relu=0)
            ref['bound'] = max([int(bound['out'].max()), int(bound['x'].max())] +
                               [int((bound[k] + np.abs(i64(self.init[k]))).max()) for k in ('basis', 'root', 'bias')])
            self._ref[relu] = ref
        return self._ref[relu]


def _tmpl_int64(c, x, basis, root, bias, gout, relu):
    X = x.reshape(c.B, c.N, c.Din)
    edges = list(zip(c.src, c.dst, c.rels))
    pre = X @ root + bias
    for s, d, r in edges:
        pre[:, d] += X[:, s] @ basis[r]
    out = np.where(pre > 0, pre, 0) if relu else pre
    gpre = np.where(pre > 0, gout.reshape(pre.shape), 0) if relu else gout.reshape(pre.shape)
    gx = gpre @ root.T
    gb = np.zeros_like(basis)
    for s, d, r in edges:
        gx[:, s] += gpre[:, d] @ basis[r].T
        gb[r] += X[:, s].T @ gpre[:, d]
    flat = lambda a: a.reshape(c.B * c.N, -1)
    return dict(out=flat(out), x=flat(gx), basis=gb, root=x.T @ flat(gpre), bias=flat(gpre).sum(0))


def tmpl_forward(be, c, relu):
    et = np.asarray(c.rels, dtype=np.int64)
    x, basis, root, bias = [be.put(a) for a in (c.x, c.basis, c.root, c.bias)]
    out = be.empty((c.B * c.N, c.Dout))
    be.check(be.lib.mpqe_rgcn_template_fwd(QUERY_TYPE_IDS[c.qt], c.B, et.ctypes.data, be.ptr(x), be.ptr(basis), R, be.ptr(root),
                                           be.ptr(bias), c.Din, c.Dout, relu, be.ptr(out), be.stream), 'template fwd')
    return be.get(out)


def tmpl_backward(be, c, relu, want=OUTPUTS):
    """-> ({name: array} of the outputs in `want`, whether every pointer was 16-byte aligned); every other gradient output
    reaches the library as NULL. The mask is the oracle's output."""
    ref = c.reference(relu)
    et = np.asarray(c.rels, dtype=np.int64)
    qi = QUERY_TYPE_IDS[c.qt]
    x, basis, root, g = [be.put(a) for a in (c.x, c.basis, c.root, c.gout)]
    out = be.put(ref['out'].astype(np.float32)) if relu else None
    buf = {k: be.empty((c.B * c.N, c.Din)) if k == 'x' else be.put(c.init[k]) for k in want}
    wb = be.lib.mpqe_rgcn_template_bwd_workspace_bytes(qi, c.B, c.Din, c.Dout)
    (nch_edge, _), (nch_root, _) = plan_chunks(c.B, c.N)
    assert wb == (align_up((c.E * nch_edge + nch_root) * c.Din * c.Dout * 4, 256) +
                  bias_partial_bytes(c.B * c.N, c.Dout) + 256)                                     # the copies hold
    ws = nan_workspace(be, wb)
    p = lambda k: be.ptr(buf.get(k))
    be.check(be.lib.mpqe_rgcn_template_bwd(qi, c.B, et.ctypes.data, be.ptr(x), be.ptr(out), be.ptr(g), be.ptr(basis), R,
                                           be.ptr(root), c.Din, c.Dout, relu, p('x'), p('basis'), p('root'), p('bias'),
                                           be.ptr(ws), wb, be.stream), 'template bwd')
    return {k: be.get(b) for k, b in buf.items()}, aligned(be, x, basis, root, g, out, ws)


def check_tmpl_grads(c, relu, got, want):
    ref = c.reference(relu)
    assert set(got) == set(want)
    for k in want:
        same(got[k], ref[k] + (0 if k == 'x' else i64(c.init[k])), 'grad_%s of %s' % (k, '+'.join(want)))


def check_tmpl(be, c, relu):
    ref = c.reference(relu)
    assert ref['bound'] < 2 ** 24           # every sum below is exact in float32, in any order
    same(tmpl_forward(be, c, relu), ref['out'], 'out')
    got, al = tmpl_backward(be, c, relu)
    check_tmpl_grads(c, relu, got, OUTPUTS)
    unused = sorted(set(range(R)) - set(c.rels))
    assert unused and not ref['basis'][unused].any()        # a relation of no template edge keeps what it held
    return al


# ------------------------------------------------------------------------------------------ C: template, chunk regimes
#            B: ((nch_edge, ch_edge), (nch_root, ch_root)) for N = 4
TMPL_B = {129: ((2, 96), (5, 128)),             # the smallest B with two chunks per edge slot
          160: ((2, 96), (5, 128)),             # B % 32 == 0: LD_FAST with a second chunk
          1024: ((8, 128), (32, 128)),          # the root slot reaches its 32 chunks uncapped
          1025: ((9, 128), (26, 160)),          # the root slot's cap: chunks longer than 128 rows
          2048: ((16, 128), (32, 256)),         # the edge slots reach their 16 chunks uncapped
          2049: ((13, 160), (29, 288)),         # both caps
          2560: ((16, 160), (32, 320))}
# name: (query type, relation of each template edge)
TMPL_TYPES = {'N2': ('1-chain', [2]),
              'N3': ('2-inter', [3, 1]),
              'N4_distinct': ('3-inter_chain', [2, 0, 3]),
              'N4_equal': ('3-inter_chain', [1, 1, 1])}     # three slots' chunks summed into one relation's matrix
# The three-edge type with distinct relations runs every B; the other three run at the smallest two-chunk B, at the
# LD_FAST one and under both caps. Every case runs on both backends: the emulator's slowest is B = 2560 at 64 x 64, 4 s.
TMPL_CASES = [(t, B, d) for t in TMPL_TYPES for B in sorted(TMPL_B) for d in DIMS if t == 'N4_distinct' or B in (129, 160, 2049)]


def tmpl_case(name, B, dims):
    qt, rels = TMPL_TYPES[name]
    return cached(('tmpl', name, B, dims), lambda: TmplCase(qt, rels, B, dims, seed=300 + B % 83 + dims[0] + len(name)))


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('name,B,dims', TMPL_CASES, ids=case_id)
def test_template_chunk_regimes(be, name, B, dims, relu):
    """mpqe_rgcn_template_fwd / _bwd with several chunks per edge slot and per root slot, the two counts far apart (the
    early return of rgcn_tmpl_grad_w_kernel for c >= nch), under the 16-chunk and the 32-chunk cap, and
    rgcn_tmpl_reduce_w_kernel summing the chunks of three slots into one relation. Emulator time of the slowest case
    (B = 2560, three edges, 64 x 64): 4 s."""
    c = tmpl_case(name, B, dims)
    edge, root = plan_chunks(B, c.N)
    assert c.N == {'N2': 2, 'N3': 3}.get(name, 4) and c.E == c.N - 1
    if c.N == 4:
        assert (edge, root) == TMPL_B[B]
    # the grid is root[0] chunks wide: the workgroups of the edge slots beyond edge[0] leave early
    assert edge == plan_chunks(B, 4)[0] and 1 < edge[0] < root[0]
    assert (edge[1] > 128) == (B > 2048) and (root[1] > 128) == (B * c.N > 4096)        # the 16-chunk and the 32-chunk cap
    assert 0 < last_chunk(B, edge) <= edge[1] and 0 < last_chunk(B * c.N, root) <= root[1]
    assert check_tmpl(be, c, relu)
    assert tmpl_grad_w_mode(B, *dims) == (SCALAR if dims == (5, 3) else FAST if dims == (64, 64) and B % 32 == 0 else PRED)
    if dims == (64, 64):
        assert (tmpl_grad_w_mode(B, *dims) == FAST) == (B in (160, 1024, 2048, 2560))


@pytest.mark.parametrize('dims', DIMS, ids=dims_id)
@pytest.mark.parametrize('absent', OUTPUTS)
def test_template_outputs_absent_in_turn(be, absent, dims):
    """grad_x, grad_basis, grad_root and grad_bias each NULL in turn at B = 160 (two chunks per edge slot, five of the
    root slot; LD_FAST at 64 x 64), relu = 1: the outputs that are present are exact."""
    c = tmpl_case('N4_distinct', 160, dims)
    assert plan_chunks(160, c.N) == ((2, 96), (5, 128))
    assert c.reference(1)['bound'] < 2 ** 24
    want = tuple(k for k in OUTPUTS if k != absent)
    got, _ = tmpl_backward(be, c, 1, want)
    check_tmpl_grads(c, 1, got, want)
