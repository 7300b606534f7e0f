"""Every buffer whose size the library dictates (the workspaces, plans and descriptor blocks of the mpqe_*_bytes functions of
include/mpqe_amd.h) held to exactly that size, between fences, whatever it holds when the call starts.

The suite's drivers allocate such buffers through `be.nbytes(n)` (tests/kernel_backend.py): n // 4 + 64 zeroed floats, often
256 bytes more for rounding the pointer up. Here the same drivers run on `Exact`, a backend that wraps the real one:

  * `nbytes` hands out tests/fenced.py's fenced_bytes(): a view of exactly the byte count the library returned (the driver's
    own `+ 256`, declared per driver as `pad`, is taken off again, and the request must then be a size the library gave),
    256-byte aligned so that the driver's rounding moves nothing, filled with one of fenced.FILLS;
  * the library is wrapped too: the size functions are recorded, and every call that takes such a buffer as a
    (pointer, size_t) pair is first made with `size - 1`, once per buffer: MPQE_ERR_WORKSPACE, and not one bit of anything
    the driver allocated -- operands, outputs (handed out holding the fence pattern), the buffers, their fences -- may
    change;
  * each such buffer in turn starts 4 bytes past its boundary. A call that takes it must give the bits of the aligned run,
    or refuse (MPQE_ERR_INVALID_ARG / MPQE_ERR_WORKSPACE) having written nothing; where the header asks for an aligned
    buffer it must refuse.

A driver is run once per fill. It checks its outputs against its own float64 reference at its own tolerance, as it does in
its own module; afterwards every array it allocated, inputs and outputs alike, must be bit-equal to the first fill's (except
the outputs the library sums with fp32 atomics, named per case), every fence intact. Nothing here sets a tolerance.

Both backends: the host emulator (`emu`) and the gfx950 library (`hip`, marked gpu).
"""
import numpy as np
import pytest

from mpqe_amd import _capi
from tests.fenced import FILLS, FLOAT_FENCE_BITS, assert_fence_intact, fenced_bytes

ERR_INVALID_ARG, ERR_WORKSPACE = -1, -3


@pytest.fixture(scope='module', params=['emu', pytest.param('hip', marks=pytest.mark.gpu)])
def be(request):
    from tests import kernel_backend
    if request.param == 'emu':
        return kernel_backend.EmuBackend()
    return kernel_backend.HipBackend()


class Refused(Exception):
    """A call on misaligned buffers came back MPQE_ERR_INVALID_ARG / MPQE_ERR_WORKSPACE, having written nothing."""


class _Lib(object):
    def __init__(self, owner, lib):
        self._owner, self._lib = owner, lib

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        proto = _capi.PROTOTYPES.get(name)
        if proto is None:
            return fn
        if name.endswith('_bytes'):
            def size(*args):
                n = int(fn(*args))
                self._owner.sizes[n] = name
                return n
            return size
        if proto[0] is not _capi.I:
            return fn
        return lambda *args: self._owner.call(name, fn, proto[1], list(args))


class Exact(object):
    """The backend `be` with exact-size, fenced, pre-filled library buffers (module docstring)."""

    def __init__(self, be, fill, pad=0, misalign=0, only=None, short=False):
        """misalign, only: the `only`-th library-sized buffer the driver asks for (all of them: None) starts `misalign` bytes
        past its boundary"""
        self.be, self.fill, self.pad, self.misalign, self.only, self.short = be, fill, pad, misalign, only, short
        self.name, self.lib = be.name, _Lib(self, be.lib)
        self.sizes = {}             # byte count -> the size function that returned it
        self.buffers = []           # (view, size function)
        self.by_id, self.by_token = {}, {}
        self.arrays = []            # everything else the driver allocated
        self.refusals = {}          # entry point -> refused short calls
        self.sized_calls = set()

    def __getattr__(self, name):    # torch, dev, stream, get, check
        return getattr(self.be, name)

    # ---- allocation
    def _track(self, a):
        self.arrays.append(a)
        return a

    def put(self, a):
        return self._track(self.be.put(a))

    def _aligned(self, shape, dtype, value):
        """A 256-byte aligned array (a view: helpers that place data by the address they are given then place it alike in
        every run, and the runs can be compared bit for bit)."""
        dtype = np.dtype(dtype)
        n = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        raw = self.be.zeros((n + 256,), np.uint8)
        skip = (-self.be.ptr(raw)) % 256
        if self.name == 'emu':
            a = raw[skip:skip + n].view(dtype).reshape(shape)
            a[...] = value
        else:
            a = raw[skip:skip + n].view(getattr(self.be.torch, dtype.name)).reshape(shape)
            a.fill_(value)
        return self._track(a)

    def zeros(self, shape, dtype=np.float32):
        return self._aligned(shape, dtype, 0)

    def empty(self, shape, dtype=np.float32, fill=None):
        if fill is None:
            fill = float('nan') if np.issubdtype(np.dtype(dtype), np.floating) else -7
        a = self._aligned(shape, dtype, fill)
        if np.isnan(fill) and np.dtype(dtype) == np.float32:      # an output: the fence pattern, bit for bit
            bits = np.array(FLOAT_FENCE_BITS[4], dtype=np.uint32).view(np.int32)[()]
            if self.name == 'emu':
                a.view(np.int32)[...] = bits
            else:
                a.view(self.be.torch.int32).fill_(int(bits))
        return a

    def _addr(self, view):
        if self.name == 'emu':
            return view.ctypes.data
        return view._base.data_ptr() + view.storage_offset()       # (an empty view has no data_ptr of its own)

    def nbytes(self, n, fill=None):
        exact = int(n) - self.pad
        assert exact in self.sizes, '%d bytes asked for: not %d more than any size the library returned (%s)' % (
            n, self.pad, sorted(self.sizes))
        mis = self.misalign if self.only in (None, len(self.buffers)) else 0
        view = fenced_bytes(self.be, exact, fill or self.fill, align=256, misalign=mis)
        real = self._addr(view)
        token = real - mis                  # what the driver sees: aligned, so that its own rounding up moves nothing
        self.buffers.append((view, self.sizes[exact]))
        self.by_id[id(view)] = token
        self.by_token[token] = (real, exact)
        return view

    def ptr(self, a):
        if a is not None and id(a) in self.by_id:
            return self.by_id[id(a)]
        return self.be.ptr(a)

    # ---- the calls
    def _image(self, a):
        if self.name == 'emu':
            whole = a if a.base is None else a.base
            return np.array(whole).tobytes()
        whole = a if a._base is None else a._base
        return whole.cpu().numpy().tobytes()

    def snapshot(self):
        if self.name != 'emu':
            self.be.torch.cuda.synchronize()
        return [self._image(a) for a in self.arrays] + [self._image(v) for v, _ in self.buffers]

    def assert_unchanged(self, before, what):
        after = self.snapshot()
        n = len(self.arrays)
        for i, (x, y) in enumerate(zip(before, after)):
            assert x == y, '%s wrote into %s' % (what, 'array %d of the driver' % i if i < n else
                                                  'the %s buffer or its fences' % self.buffers[i - n][1])

    def call(self, name, fn, argtypes, args):
        pairs, off = [], False            # off: a buffer of this call is not where its alignment puts it
        for i, a in enumerate(args):
            if isinstance(a, int) and a in self.by_token and argtypes[i] is _capi.P:
                real, exact = self.by_token[a]
                args[i] = real
                off = off or real != a
                if i + 1 < len(args) and argtypes[i + 1] is _capi.Z:
                    assert args[i + 1] == exact, '%s: the driver passes %d bytes for a buffer of %d' % (name, args[i + 1], exact)
                    pairs.append(i)
        if pairs:
            self.sized_calls.add(name)
        before = self.snapshot() if ((pairs and self.short) or off) else None
        if self.short:
            for i in pairs:
                short = list(args)
                short[i + 1] -= 1
                st = fn(*short)
                what = '%s with argument %d one byte short' % (name, i + 1)
                assert st == ERR_WORKSPACE, '%s returned %d, not MPQE_ERR_WORKSPACE' % (what, st)
                self.assert_unchanged(before, what)
                self.refusals[name] = self.refusals.get(name, 0) + 1
        st = fn(*args)
        if off and st in (ERR_INVALID_ARG, ERR_WORKSPACE):
            self.assert_unchanged(before, '%s, refused (%d) on misaligned buffers,' % (name, st))
            raise Refused(name)
        return st

    # ---- afterwards
    def assert_fences(self):
        for view, what in self.buffers:
            assert_fence_intact(self.be, view, what)

    def images(self):
        """the arrays themselves (not the allocations behind them, whose alignment padding differs from run to run)"""
        return [np.ascontiguousarray(self.be.get(a)).tobytes() for a in self.arrays]


WORST = {}      # (backend, group) -> the worst |got - reference| any driver's assert_allclose saw here; printed at the end


class _Recorded(object):
    """While a driver runs, np.testing.assert_allclose (where every `close` of the suite ends) also notes its worst absolute
    difference under the group's name. It asserts what it asserted."""

    def __init__(self, key):
        self.key = key

    def __enter__(self):
        self.plain = np.testing.assert_allclose

        def noting(actual, desired, *args, **kwargs):
            a, d = np.asarray(actual, dtype=np.float64), np.asarray(desired, dtype=np.float64)
            if a.size and a.shape == d.shape and np.isfinite(a).all() and np.isfinite(d).all():
                note(self.key, np.abs(a - d).max())
            return self.plain(actual, desired, *args, **kwargs)
        np.testing.assert_allclose = noting

    def __exit__(self, *exc):
        np.testing.assert_allclose = self.plain


def note(key, err):
    WORST[key] = max(WORST.get(key, 0.0), float(err))


@pytest.fixture(scope='module', autouse=True)
def worst_errors():
    yield
    for (name, group), err in sorted(WORST.items()):
        print('worst absolute error against the float64 reference, %s / %s: %.3g' % (name, group, err))


BITWISE = ('row plans', 'KG answers', 'KG sampling', 'GQE embed + ranking')       # groups whose drivers compare bits alone: nothing to record


def sweep(be, driver, group, pad=0, atomic=(), must_refuse=(), each=True):
    with _Recorded((be.name, group)):
        out = _sweep(be, driver, pad, atomic, must_refuse, each)
    assert group in BITWISE or (be.name, group) in WORST, 'no float comparison of the driver was seen'
    return out


def _sweep(be, driver, pad, atomic, must_refuse, each):
    """`driver(backend)` once per fill on exact-size fenced buffers (the 'nan' run also makes every sized call one byte
    short first), then once per library-sized buffer with that buffer alone 4 bytes off its boundary.
    atomic: indices, in allocation order, of the arrays that the library sums with fp32 atomics; the driver checks those
    against its reference, their bits are free. must_refuse: the size functions whose buffers the header wants aligned --
    4 bytes off, a call that takes one must be refused; the others may be refused or give the aligned run's bits.
    each = False (a second case of an entry point whose buffers another case takes one by one): one run with all of them off.
    -> {size function: outcomes}"""
    first = names = None
    for fill in FILLS:
        xb = Exact(be, fill, pad=pad, short=(fill == 'nan'))
        driver(xb)
        xb.assert_fences()
        assert xb.buffers and xb.sized_calls, 'the driver gave the library no sized buffer'
        if xb.short:
            assert set(xb.refusals) == xb.sized_calls
        images = xb.images()
        if first is None:
            first, names = images, [name for _, name in xb.buffers]
        assert len(images) == len(first) and [name for _, name in xb.buffers] == names
        for i, (x, y) in enumerate(zip(first, images)):
            assert i in atomic or x == y, 'array %d of the driver depends on what the buffers held: %s differs from %s' % (
                i, fill, list(FILLS)[0])
    assert set(must_refuse) <= set(names), 'no buffer of %s' % sorted(set(must_refuse) - set(names))
    outcomes = {}
    for j, name in enumerate(names if each else [' and '.join(names)]):
        xb = Exact(be, 'nan', pad=pad, misalign=4, only=j if each else None)
        try:
            driver(xb)
        except Refused:
            xb.assert_fences()
            outcomes.setdefault(name, []).append('refused')
            continue
        assert name not in must_refuse and (each or not must_refuse), 'the header asks for an aligned %s buffer: 4 bytes off should have been refused' % name
        xb.assert_fences()
        for i, (x, y) in enumerate(zip(first, xb.images())):
            assert i in atomic or x == y, 'array %d of the driver: other bits with the %s buffer 4 bytes off' % (i, name)
        outcomes.setdefault(name, []).append('same bits')
    return outcomes


# ------------------------------------------------------------------------------------------------ the harness itself
@pytest.mark.parametrize('fill', list(FILLS))
@pytest.mark.parametrize('nbytes,misalign', [(0, 0), (1, 0), (255, 4), (256, 0), (5000, 4), (70001, 12)])
def test_fenced_bytes(be, nbytes, misalign, fill):
    v = fenced_bytes(be, nbytes, fill, misalign=misalign)
    base = v.base if be.name == 'emu' else v._base
    start = (v.ctypes.data - base.ctypes.data) if be.name == 'emu' else int(v.storage_offset())
    assert int(v.shape[0]) == nbytes and (be.ptr(base) + start) % 256 == misalign
    assert start >= max(nbytes, 4096) and int(base.shape[0]) - start - nbytes >= max(nbytes, 4096)
    got = be.get(v)
    assert got.dtype == np.uint8 and (got == np.resize(FILLS[fill], nbytes)).all()
    assert_fence_intact(be, v, 'untouched')
    if nbytes and FILLS[fill].size == 4:
        assert be.get(v[:4 * (nbytes // 4)]).view(np.uint32).tolist() == [int(FILLS[fill].view('<u4')[0])] * (nbytes // 4)
    for where in range(4):          # one byte on either side, and the far ends
        w = fenced_bytes(be, nbytes, fill, misalign=misalign)
        wbase = w.base if be.name == 'emu' else w._base
        wstart = (w.ctypes.data - wbase.ctypes.data) if be.name == 'emu' else int(w.storage_offset())
        at = (wstart - 1, wstart + nbytes, 0, int(wbase.shape[0]) - 1)[where]
        wbase[at] = int(wbase[at]) ^ 0x10
        with pytest.raises(AssertionError):
            assert_fence_intact(be, w, 'poked')


# ------------------------------------------------------------------------------------------------ template layer backward
@pytest.mark.parametrize('shape', [(5, 16, 16, 4), (67, 40, 24, 5), (5, 40, 24, 5), (67, 16, 16, 4)],
                         ids=lambda s: 'B%d_%dx%d' % s[:3])
def test_template_bwd_workspace(be, shape):
    from tests import test_operand_bounds as tob
    sweep(be, lambda xb: tob.test_template_layer_fenced(xb, '3-inter_chain', shape, 'none'), 'template layer',
          must_refuse={'mpqe_rgcn_template_bwd_workspace_bytes'})


# ------------------------------------------------------------------------------------------------ general layer
# include/mpqe_amd.h: "workspace (forward and backward): 16-byte aligned, MPQE_ERR_INVALID_ARG otherwise"
GENERAL_ALIGNED = {'mpqe_rgcn_general_workspace_bytes'}


@pytest.mark.parametrize('case,slots', [('heavy_10x6', None), ('heavy_40x24', None), ('register_128x64', None),
                                        ('register_128x64', 16)])
def test_general_layer_buffers(be, case, slots, request):
    """tests/test_operand_bounds.py's driver: 130 nodes, 400 edges (E + Nn = 530 message rows: eight 64-row tiles and 18
    rows), a relation without an edge; plan, plan workspace and both layer workspaces exact. GEN_SLOTS = 16: the persistent
    grid of 16 workgroups walks the row tiles."""
    from tests import test_operand_bounds as tob
    if slots is not None:
        be.lib.mpqe_debug_option(b'GEN_SLOTS', slots, 1)
        request.addfinalizer(lambda: be.lib.mpqe_debug_option(b'GEN_SLOTS', 0, 0))
    sweep(be, lambda xb: tob.test_general_layer_fenced(xb, case, 'none', 1), 'general layer', must_refuse=GENERAL_ALIGNED)


def test_general_layer_buffers_heavy_relation(be):
    """tests/test_kernels.py's heavy-relation graph (50 nodes, 700 edges, dims 10 -> 6) on its run_general driver, which
    also allocates the ReLU bit mask through nbytes."""
    from tests import test_kernels as tk
    sweep(be, tk.test_general_layer_heavy_relation_and_odd_dims, 'general layer', must_refuse=GENERAL_ALIGNED)


@pytest.mark.parametrize('slots', [None, 16])
def test_general_layer_buffers_64_tiles(be, slots, request):
    """300 nodes, 1100 edges, 128 -> 64, ReLU: the mask words sized by mpqe_rgcn_general_mask_bytes; 1400 message rows are
    21 tiles and 56 rows, not a whole group of 8 tiles either."""
    from tests import test_kernels as tk
    sweep(be, lambda xb: tk.test_general_layer_dims_of_64_register_tiles(xb, 1, (128, 64), slots, request), 'general layer',
          must_refuse=GENERAL_ALIGNED)


# ------------------------------------------------------------------------------------------------ dense layer backward
@pytest.mark.parametrize('overwrite', [1, 0])
@pytest.mark.parametrize('shape', [(70, 48, 20, 16, 8), (1, 2, 1, 0, 0), (257, 96, 60, 32, 32), (96, 64, 64, 64, 0)],
                         ids=lambda s: '%dx%dx%d_ld+%d_off%d' % s)
def test_linear_bwd_workspace(be, shape, overwrite):
    from tests import test_operand_bounds as tob
    rows, din, dout, pad, off = shape
    c = tob.DenseCase(rows, din, dout, din + pad, off, 1, tob.seed_of(shape))
    sweep(be, lambda xb: tob.dense_bwd(xb, c, overwrite), 'dense layer', must_refuse={'mpqe_linear_bwd_workspace_bytes'})


# ------------------------------------------------------------------------------------------------ scatter
@pytest.mark.parametrize('size', [1, 64, 65])
def test_scatter_mean_workspace(be, size):
    """tests/test_op_edges.py's check_scatter: 150 rows of width 5 over `size` segments, every third segment empty. The
    workspace holds the mean's counts (add and max take none). `out`, array 0 of the driver, is summed with fp32 atomics."""
    from tests import test_op_edges as toe
    rng = np.random.RandomState(size)
    n, D = 150, 5
    live = np.array([s for s in range(size) if s % 3 != 1 or size == 1], dtype=np.int64)
    index = live[rng.randint(0, live.size, size=n)]
    src = rng.randn(n, D).astype(np.float32)
    g = rng.randn(size, D).astype(np.float32)
    def driver(xb):
        assert toe.check_scatter(xb, 'mean', src, index, size, g) == 0, 'the error word'
    sweep(be, driver, 'scatter mean', atomic=(0,))


# ------------------------------------------------------------------------------------------------ LayerNorm + ReLU backward
@pytest.mark.parametrize('rows', [1, 5, 9])
@pytest.mark.parametrize('D', [2, 65, 260])
def test_layernorm_bwd_workspace(be, D, rows):
    from tests import test_op_edges as toe
    sweep(be, lambda xb: toe.test_layernorm_relu_edges(xb, D, rows, 1), 'LayerNorm', pad=256)


# ------------------------------------------------------------------------------------------------ ranking
# Q 1 and 65 (a second block of queries); N 1, 64, 65 (one tile, one tile + a row) and 8300 (130 tiles, 3 per strip, 44
# strips); k 0, 1, 16 | 17, 64 | 65, 128: the edges of the three candidate-list variants
RANK_SHAPES = [(1, 1, 16, 1), (65, 64, 16, 16), (65, 65, 10, 17), (1, 8300, 8, 64), (3, 8300, 8, 65), (65, 257, 48, 128),
               (65, 65, 16, 0)]
_RANK = {}


def rank_problem(shape, dot):
    from tests import test_rank as tr, test_rank_dot as td
    key = (shape, dot)
    if key not in _RANK:
        Q, N, D, k = shape
        mod = td if dot else tr
        rng, q, table, target = mod.make(500 + Q + N + k, Q, N, D)
        _RANK[key] = (q, table, target, tr.random_excl(rng, Q, N, target, 40), mod.truth(q, table))
    return _RANK[key]


@pytest.mark.parametrize('with_excl', [False, True], ids=['plain', 'exclusions'])
@pytest.mark.parametrize('shape', RANK_SHAPES, ids=lambda s: 'Q%d_N%d_D%d_k%d' % s)
def test_rank_workspace(be, shape, with_excl):
    """tests/test_rank.py's run + check_topk / check_rank: the norms, the target scores and rows, both counters and the
    Q * S * k candidate lists in a workspace of exactly mpqe_rank_workspace_bytes."""
    from tests import test_rank as tr
    q, table, target, excl, s64 = rank_problem(shape, False)
    excl = excl if with_excl else None
    k = shape[3]

    def driver(xb):
        out = tr.run(xb, q, table, target, excl, k)
        assert out['err'] == 0
        if k:
            tr.check_topk(out, s64, excl, k)
        tr.check_rank(out, s64, target, excl)
        note((xb.name, 'ranking'), np.abs(out['tscore'] - s64[np.arange(len(target)), target]).max())
    sweep(be, driver, 'ranking')


@pytest.mark.parametrize('shape', [(65, 65, 10, 17), (3, 8300, 8, 65)], ids=lambda s: 'Q%d_N%d_D%d_k%d' % s)
def test_rank_scored_workspace(be, shape):
    """mpqe_rank_entities_scored by the dot product (tests/test_rank_dot.py's run), with exclusion lists."""
    from tests import test_rank as tr, test_rank_dot as td
    q, table, target, excl, s64 = rank_problem(shape, True)
    k = shape[3]

    def driver(xb):
        out = td.run(xb, q, table, target, excl, k)
        assert out['err'] == 0
        td.check_topk(out, s64, excl, k)
        td.check_rank(out, s64, target, excl)
        note((xb.name, 'ranking by dot'), np.abs(out['tscore'] - s64[np.arange(len(target)), target]).max())
    sweep(be, driver, 'ranking by dot')


# ------------------------------------------------------------------------------------------------ GQE
# B 1, 17, 33: p_rows is not its own round-up to 16 rows; D 16 and 48 (one and three column blocks)
@pytest.mark.parametrize('qt,D,B,inter', [('3-inter_chain', 16, 1, 'min'), ('3-inter_chain', 48, 17, 'min'),
                                          ('3-inter_chain', 16, 33, 'min'), ('2-chain', 48, 17, 'mean'),
                                          ('2-chain', 16, 33, 'mean'), ('3-inter', 48, 33, 'mean')])
def test_gqe_workspace(be, qt, D, B, inter):
    """tests/test_gqe_kernels.py's check (forward with saved states, backward, the float64 oracle). The header asks for a
    256-byte aligned workspace (include/mpqe_amd.h, mpqe_gqe_fwd: "mpqe_gqe_workspace_bytes, 256-byte aligned"): 4 bytes
    off must be refused."""
    from tests import test_gqe_kernels as tg
    prob, o, scores = tg.settled(qt, D, B, inter)
    sweep(be, lambda xb: tg.check(xb, prob, o, scores), 'GQE', pad=256, must_refuse={'mpqe_gqe_workspace_bytes'})


# the two vector operators (programme int [7]): their sites own other blocks of gqe_plan's layout -- X only under the scale
# operator, and one partial row per 16-row workgroup, (Rp16 / 16) * dim floats rounded up to 64. B 17 / 33: two and three
# partial rows in the intersection forms, many in the chain forms (p_rows = B + the negatives)
@pytest.mark.parametrize('dec,qt,D,B,inter', [('transe', '3-inter_chain', 48, 17, 'min'), ('transe', '2-chain', 16, 33, 'mean'),
                                              ('bilinear-diag', '3-inter_chain', 16, 33, 'min'),
                                              ('bilinear-diag', '2-chain', 48, 17, 'mean'),
                                              # (two translate sites: two blocks of seven partial rows side by side)
                                              ('transe', '2-chain', 48, 17, 'mean')])
def test_gqe_vector_workspace(be, dec, qt, D, B, inter):
    """tests/test_gqe_vec_kernels.py's check (gqe_vec_common.call) under the translate and the scale operator; the diagonal
    chain also scores by the dot product. The workspace is 256-byte aligned by the header, as in test_gqe_workspace."""
    from tests import test_gqe_vec_kernels as tv
    prob, o, scores = tv.settled(dec, qt, D, B, inter)
    sweep(be, lambda xb: tv.check(xb, prob, o, scores), 'GQE vectors', pad=256, must_refuse={'mpqe_gqe_workspace_bytes'})


@pytest.mark.parametrize('qt,inter', [('2-chain', 'mean'), ('3-inter_chain', 'min')])
def test_gqe_embed_then_rank(be, qt, inter):
    """tests/test_gqe_embed_kernels.py's embed_then_rank. mpqe_gqe_embed takes NO workspace (include/mpqe_amd.h: "no
    workspace, no states"): there is nothing of its own to size, fill or cut short. What is held to its size here is the
    ranking workspace its rows go into, and the rows themselves are among the arrays compared bit for bit across the fills."""
    from tests import test_gqe_embed_kernels as te
    sweep(be, lambda xb: te.embed_then_rank(xb, qt, inter), 'GQE embed + ranking')


# ------------------------------------------------------------------------------------------------ fused step
_STEP = {}


def step_problem(D, readout, adaptive, L):
    from tests import test_step as ts
    key = (D, readout, adaptive, L)
    if key not in _STEP:
        prob = ts.make_problem(11, D, L, False, ts.MIXES['all7'], readout, adaptive)
        _STEP[key] = (prob, ts.oracle_step(prob[3], prob[5], prob[4], prob[6], 1.0))
    return _STEP[key]


# D 32: the level form (no touch plan: the table gradients are fp32 atomics); D 64: the chain form
@pytest.mark.parametrize('D,readout,adaptive,L,touch', [(32, 'mp', True, 3, False), (64, 'mp', True, 3, 'step'),
                                                        (64, 'mp', True, 3, 'pack'), (64, 'mp', True, 3, False),
                                                        (64, 'mlp', False, 2, 'step'), (64, 'mp', True, 3, 'ex')],
                         ids=lambda v: str(v))
def test_step_buffers(be, D, readout, adaptive, L, touch):
    """tests/test_step.py's run_step on the seven-template mix with workspace, descriptor block, touch plan and touch
    workspace exact (its `alloc` option), checked as test_fused_step_matches_oracle checks it.
    include/mpqe_amd.h, MPQE_STEP_BUILD_TOUCH: "The plan buffer must be ZERO-FILLED once, before its first use as an
    output" -- the touch plan therefore starts as zeros whatever the fill; the fills apply to the two workspaces and the
    descriptor block."""
    from tests import test_step as ts
    (schema, mode_ids, rel_ids, params, node_map, cfg, batches), (ref_loss, ref_per, ref_sp, ref_sn) = \
        step_problem(D, readout, adaptive, L)
    atomic = set()
    # 'ex': mpqe_step_forward_backward_ex -- batch weights read from device scalars, the query embeddings written out
    ex, touch = touch == 'ex', 'step' if touch == 'ex' else touch

    def driver(xb):
        def place(be_, name, array):
            a = be_.put(array)
            if name.startswith('G.enc.feat-') and not touch:
                atomic.add(len(xb.arrays) - 1)
            return a
        PLAN_MUST_START_ZERO_FILLED = 'zeros'

        def alloc(be_, name, nbytes):
            return be_.nbytes(nbytes, fill=PLAN_MUST_START_ZERO_FILLED if name == 'touch' else None)
        qs = [] if ex else None
        loss, sp, sn, grads, err = ts.run_step(xb, schema, mode_ids, params, node_map, cfg, batches, 1.0, touch=touch,
                                               place=place, alloc=alloc, dev_weights=ex, query_out=qs)
        assert err == 0
        if ex:
            q_ref = np.concatenate([ts.ref_cpu.encode_queries(params, cfg, node_map, b['formula'], b['col']).detach().numpy()
                                    for b in batches])
            np.testing.assert_allclose(qs[0], q_ref, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(sp, ref_sp, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(sn, ref_sn, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(loss[1:], ref_per, rtol=1e-5, atol=1e-6)
        if not ex:      # (loss[0] is formed with the host weights alone, which the device weights halve here)
            np.testing.assert_allclose(loss[0], ref_loss, rtol=1e-5, atol=1e-6)
        for k, p in params.items():
            ref = np.zeros(tuple(p.shape), np.float32) if p.grad is None else p.grad.numpy()
            np.testing.assert_allclose(grads[k], ref, rtol=1e-4, atol=2e-6, err_msg=k)
    # (include/mpqe_amd.h: "workspace must be 256-byte aligned", `desc` and `touch` "256-byte aligned")
    sweep(be, driver, 'fused step', atomic=atomic,
          must_refuse={'mpqe_step_workspace_bytes', 'mpqe_step_desc_bytes'} | ({'mpqe_step_touch_bytes'} if touch else set()),
          each=readout == 'mp')           # (the learned readout: the same entry point, all its buffers off at once)


# ------------------------------------------------------------------------------------------------ row plans
# n 1, 255, 256, 257: one key, a workgroup of 256 less one, whole, and one more; runs of equal keys throughout
ROW_PLANS = {1: ((1,), 0), 255: ((5,) * 51, 0), 256: ((4,) * 64, 0), 257: ((4,) * 64, 1)}


@pytest.mark.parametrize('D', [4, 16])
@pytest.mark.parametrize('n', list(ROW_PLANS))
def test_rows_plan_and_table_rows_sum_buffers(be, n, D, monkeypatch):
    """tests/test_exchange_kernels.py's _build_plan (the plan against numpy's stable sort) and _sum_call (the tables against
    _sum_reference, bit for bit), its random-bits plan and workspace (_garbage: rounded up, 256 bytes more) replaced by
    exact ones."""
    from tests import test_exchange_kernels as tek
    monkeypatch.setattr(tek, '_garbage', lambda be_, rng, nbytes: be_.nbytes(nbytes))
    runs, tail = ROW_PLANS[n]
    rng0 = np.random.RandomState(n + D)
    keys = tek._run_keys(rng0, runs, tail)
    assert len(keys) == n
    rows = rng0.randn(n, D).astype(np.float32)
    tables = [rng0.randn(r, D).astype(np.float32) for r in tek.SUM_ROWS]
    want = [tek._sum_reference(keys, rows, tables, tek.SUM_ROW_BITS, store) for store in (0, 1)]

    def driver(xb):
        d_keys = tek._put_keys(xb, keys)
        plan, _ = tek._build_plan(xb, d_keys, n, tek.SUM_ROW_BITS, tek.SUM_ROW_BITS + 5, None, keys)
        d_rows = tek._at(xb, rows)
        for store in (0, 1):
            d_tabs = [tek._at(xb, t) for t in tables]
            assert tek._sum_call(xb, plan, n, d_rows, D, d_tabs, store) == tek.OK
            for t in range(2):
                np.testing.assert_array_equal(tek._bits(xb, d_tabs[t]), want[store][t].view(np.uint32))
    sweep(be, driver, 'row plans')


@pytest.mark.parametrize('D', [4, 16])
@pytest.mark.parametrize('n', [1, 40, 255, 256, 257])
def test_adam_rows_step_on_an_exact_plan(be, n, D):
    """tests/test_guarded_update.py: a plan of n keys in exact buffers, then mpqe_adam_rows_step and its guarded form (which
    take the plan without a byte count)."""
    from tests import test_guarded_update as tgu
    sweep(be, lambda xb: tgu.test_rows_guarded_update(xb, D, n), 'row plans', pad=256)


# ------------------------------------------------------------------------------------------------ KG answers, KG sampling
# Their kernel tests already start the workspace from random bits, 4 / 8 bytes off a 256-byte boundary, but give it 4 / 8
# bytes more than asked and ~500 bytes of zeros behind: neither exact nor fenced. Here it is both.
def _exact_workspace(module, monkeypatch):
    """module._workspace(be, rng, need, misalign), the one place where the module's calls get their workspace"""
    monkeypatch.setattr(module, '_workspace', lambda be_, rng, need, misalign: be_.nbytes(need))


@pytest.mark.parametrize('qt,Q', [('3-inter_chain', 17), ('3-chain_inter', 3), ('1-chain', 1)])
def test_kg_answers_workspace(be, qt, Q, monkeypatch):
    """tests/test_kg_kernels.py: the seven-type world, bitmaps in LDS and in the workspace (MPQE_KG_GLOBAL_BITS)."""
    from tests import test_kg_kernels as tkk
    _exact_workspace(tkk, monkeypatch)
    sweep(be, lambda xb: tkk.test_all_seven_query_types(xb, qt, Q), 'KG answers')


def test_kg_answers_workspace_wide_bitmaps(be, monkeypatch):
    """a mode of 2049 rows: 65 words a bitmap"""
    from tests import test_kg_kernels as tkk
    _exact_workspace(tkk, monkeypatch)
    sweep(be, lambda xb: tkk.test_word_edges(xb, 2049), 'KG answers')


@pytest.mark.parametrize('qt', [0, 5])
def test_kg_sample_workspace(be, qt, monkeypatch):
    """tests/test_kg_sample_kernels.py: the walk against its restated stream, Q 1 / 255 / 257. include/mpqe_amd.h,
    mpqe_kg_sample_queries: the workspace is "8-byte aligned" -- 4 bytes off must be refused."""
    from tests import test_kg_sample_kernels as tks
    _exact_workspace(tks, monkeypatch)
    sweep(be, lambda xb: tks.test_walk_equals_the_restated_stream(xb, qt), 'KG sampling',
          must_refuse={'mpqe_kg_sample_workspace_bytes'})


# ------------------------------------------------------------------------------------------------ peer exchange (emulated ranks)
@pytest.mark.parametrize('fill', list(FILLS))
@pytest.mark.parametrize('world,cap,n', [(1, 37, 37), (3, 4099, 4097), (8, 5000, 37), (8, 4101, 4101), (3, 64, 50)])
def test_p2p_buffers(world, cap, n, fill):
    """tests/test_parallel.py's peer_exchange (emulator only: the ranks of one process) on buffers of exactly
    mpqe_p2p_buffer_bytes. n no multiple of 4 * world, n < capacity, one rank. The call takes no byte count, so there is no
    short call to refuse. Initial state: the flag words are zero, as mpqe_p2p_alloc -- the library's own allocator, which
    clears the whole buffer -- leaves them (csrc/p2p.hip: epoch-stamped, "never cleared"; workgroup counters that return to
    zero); bucket and staging slots hold the fill."""
    from tests.kernel_backend import EmuBackend
    from tests.test_parallel import peer_exchange
    emu = EmuBackend()

    def alloc(nbytes, flags_offset):
        FLAGS_START_ZERO_AS_P2P_ALLOC_LEAVES_THEM = 0
        v = fenced_bytes(emu, nbytes, fill)
        v[flags_offset:] = FLAGS_START_ZERO_AS_P2P_ALLOC_LEAVES_THEM
        return v, v.ctypes.data
    for v in peer_exchange(emu, world, cap, n, np.random.RandomState(world + n), alloc):
        assert_fence_intact(emu, v, 'p2p buffer')
