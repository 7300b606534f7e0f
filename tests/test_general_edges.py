"""The general R-GCN layer (csrc/rgcn_general.hip) exactly at its tile, chunk and slab edges.

Every operand is a small integer stored as float32 (uniform in {-2 .. 2}) and the oracle is the same layer in numpy int64:
gather, per-relation product, np.add.at over destinations, ReLU as `pre > 0`, the four gradients behind the mask `out > 0`.
Each test asserts from its data that every output element's sum of ABSOLUTE terms -- the oracle run on the absolute values,
accumulate-mode contents included -- stays below 2^24: then every float32 product and every partial sum is an integer that
float32 holds, in whatever order a kernel adds them, MFMA or scalar. So every comparison below is an equality: one lost or
doubled message slot, slab or tile row shows, which no tolerance that float32 summation of Gaussian data needs would let it.
The ReLU mask words are compared bit by bit; exact zeros of the pre-activation are frequent with such inputs.

Runs on the host emulator (`emu`) and on the gfx950 library (`hip`, marked gpu), tests/test_kernels.py's fixture pattern.
"""
import numpy as np
import pytest

from mpqe_amd._capi import FLAG_BAD_EDGE, FLAG_BAD_RELATION

GT_BM, GEN_CHUNK = 64, 512          # csrc/gemm_core.h, csrc/rgcn_general.hip: rows of a tile, slots of a K chunk
ALL = ('x', 'basis', 'root', 'bias')
DIMS = [(64, 64), (40, 24), (5, 3)]     # register-operand kernels / LD_PRED / LD_SCALAR with Din * Dout % 4 != 0
dims_id = lambda d: '%dx%d' % d


@pytest.fixture(scope='module', params=['emu', pytest.param('hip', marks=pytest.mark.gpu)])
def be(request):
    from tests import kernel_backend
    if request.param == 'emu':
        return kernel_backend.EmuBackend()
    return kernel_backend.HipBackend()


# ------------------------------------------------------------------------------------------ data and oracle
def small_ints(rng, shape):
    return rng.randint(-2, 3, size=shape).astype(np.float32)


class Case(object):
    """One graph with its operands, the upstream gradient and the contents the accumulate-mode buffers start with."""

    def __init__(self, Nn, R, src, dst, typ, dims, seed, bad=None):
        rng = np.random.RandomState(seed)
        self.Nn, self.R, (self.Din, self.Dout) = Nn, R, dims
        Din, Dout = dims
        self.src, self.dst, self.typ = [np.asarray(a, dtype=np.int64).reshape(-1) for a in (src, dst, typ)]
        self.E = self.typ.shape[0]
        # what the plan is given; `bad` = (src, dst, typ) with out-of-range entries where the three above hold the clamped ones
        self.given = bad if bad is not None else (self.src, self.dst, self.typ)
        self.x, self.basis, self.root = small_ints(rng, (Nn, Din)), small_ints(rng, (R, Din, Dout)), small_ints(rng, (Din, Dout))
        self.bias, self.gout = small_ints(rng, (Dout,)), small_ints(rng, (Nn, Dout))
        self.init = dict(basis=small_ints(rng, (R, Din, Dout)), root=small_ints(rng, (Din, Dout)), bias=small_ints(rng, (Dout,)))
        self.counts = np.bincount(self.typ, minlength=R)[:R] if self.E else np.zeros(R, np.int64)
        self._ref = {}

    def tiles(self):
        return int(sum((int(c) + GT_BM - 1) // GT_BM for c in list(self.counts) + [self.Nn]))

    def slabs(self):
        return [(int(c) + GEN_CHUNK - 1) // GEN_CHUNK for c in list(self.counts) + [self.Nn]]

    def reference(self, relu, bias=True):
        key = (relu, bias)
        if key not in self._ref:
            i64 = lambda a: a.astype(np.int64)
            ops = [i64(a) for a in (self.x, self.basis, self.root, self.bias if bias else 0 * self.bias, self.gout)]
            ref = _layer_int64(self, *ops, relu=relu)
            # the same sums over absolute values, no term masked away: an upper bound of every partial sum in every order
            bound = _layer_int64(self, *[np.abs(a) for a in ops], relu=0)
            ref['bound'] = max([int(bound['out'].max()), int(bound['x'].max())] +
                               [int((bound[k] + np.abs(i64(self.init[k]))).max()) for k in ('basis', 'root', 'bias')
                                if bound[k].size])
            self._ref[key] = ref
        return self._ref[key]


def _layer_int64(c, x, basis, root, bias, gout, relu):
    rels = [(r, np.flatnonzero(c.typ == r)) for r in range(c.R) if c.counts[r]]
    pre = x @ root + bias
    for r, e in rels:
        np.add.at(pre, c.dst[e], x[c.src[e]] @ basis[r])
    out = np.where(pre > 0, pre, 0) if relu else pre
    gpre = np.where(pre > 0, gout, 0) if relu else gout
    gx = gpre @ root.T
    gb = np.zeros_like(basis)
    for r, e in rels:
        np.add.at(gx, c.src[e], gpre[c.dst[e]] @ basis[r].T)
        gb[r] = x[c.src[e]].T @ gpre[c.dst[e]]
    return dict(out=out, x=gx, basis=gb, root=x.T @ gpre, bias=gpre.sum(0))


def graph_by_counts(counts, Nn, seed):
    """`counts[r]` edges of relation r, endpoints uniform, in shuffled edge order."""
    rng = np.random.RandomState(seed)
    typ = rng.permutation(np.repeat(np.arange(len(counts)), counts))
    return rng.randint(0, Nn, size=typ.shape[0]), rng.randint(0, Nn, size=typ.shape[0]), typ


_cases = {}


def cached(key, make):
    """cases are built, and their oracles computed, once for both backends"""
    if key not in _cases:
        _cases[key] = make()
    return _cases[key]


# ------------------------------------------------------------------------------------------ driver
class Device(object):
    """A case's operands on one backend with its plan built. Unlike test_kernels.run_general it leaves `bias`, `out`, the
    mask words and any gradient output away when told to: NULL is what reaches the library, never a buffer."""

    def __init__(self, be, c):
        self.be, self.c = be, c
        lib = be.lib
        self.err = be.zeros((1,), np.int32)
        pb, pw = lib.mpqe_rgcn_plan_bytes(c.Nn, c.E, c.R), lib.mpqe_rgcn_plan_workspace_bytes(c.Nn, c.E, c.R)
        self.plan, pws = be.nbytes(pb), be.nbytes(pw)
        ei = be.put(np.stack([c.given[0], c.given[1]]).astype(np.int64))
        et = be.put(np.asarray(c.given[2], dtype=np.int64))
        be.check(lib.mpqe_rgcn_plan_build(be.ptr(ei), be.ptr(et), c.Nn, c.E, c.R, be.ptr(self.plan), pb, be.ptr(pws), pw,
                                          be.ptr(self.err), be.stream), 'plan')
        self.x, self.root, self.bias, self.gout = [be.put(a) for a in (c.x, c.root, c.bias, c.gout)]
        self.basis = be.put(c.basis) if c.R else None
        self.args = (be.ptr(self.plan), c.Nn, c.E, c.R)

    def flags(self):
        return int(self.be.get(self.err)[0])

    def forward(self, relu, bias=True, words=True):
        """-> (out, mask words or None), both on the device. The words start as all ones."""
        be, c = self.be, self.c
        out = be.empty((c.Nn, c.Dout))
        wf = be.lib.mpqe_rgcn_general_workspace_bytes(c.Nn, c.E, c.R, c.Din, c.Dout, 0)
        ws = be.nbytes(wf)
        mb = be.lib.mpqe_rgcn_general_mask_bytes(c.Nn, c.Dout) if relu and words else 0
        mw = None
        if mb:
            mw = be.nbytes(mb)
            (mw.view(np.int32).fill if be.name == 'emu' else mw.view(be.torch.int32).fill_)(-1)
        be.check(be.lib.mpqe_rgcn_general_fwd(*self.args, be.ptr(self.x), be.ptr(self.basis), be.ptr(self.root),
                                              be.ptr(self.bias) if bias else None, c.Din, c.Dout, relu, be.ptr(out),
                                              be.ptr(mw), be.ptr(ws), wf, be.stream), 'fwd')
        return out, mw

    def mask_bits(self, mw):
        """the words as a [Nn, Dout] array of bits: bit c % 64 of word [row][c / 64] (csrc/bias_grad.h)"""
        c = self.c
        w = np.asarray(self.be.get(mw)).view(np.uint64)[:c.Nn * (c.Dout // 64)].reshape(c.Nn, c.Dout // 64)
        return ((w[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(c.Nn, c.Dout)

    def backward(self, relu, overwrite, want=ALL, out=None, words=None):
        """-> {name: array} of the outputs in `want`; every other gradient output goes in as NULL. Overwrite mode
        writes onto NaN, accumulate mode onto the case's integer contents (grad_x is written whole in both)."""
        be, c = self.be, self.c
        shapes = dict(x=(c.Nn, c.Din), basis=(c.R, c.Din, c.Dout), root=(c.Din, c.Dout), bias=(c.Dout,))
        buf = {}
        for k in want:
            if k == 'basis' and c.R == 0:
                continue
            buf[k] = be.empty(shapes[k]) if overwrite or k == 'x' else be.put(c.init[k])
        wb = be.lib.mpqe_rgcn_general_workspace_bytes(c.Nn, c.E, c.R, c.Din, c.Dout, 1)
        ws = be.nbytes(wb)
        p = lambda k: be.ptr(buf.get(k))
        be.check(be.lib.mpqe_rgcn_general_bwd(*self.args, be.ptr(self.x), be.ptr(out), be.ptr(words), be.ptr(self.gout),
                                              be.ptr(self.basis), be.ptr(self.root), c.Din, c.Dout, relu, overwrite, p('x'),
                                              p('basis'), p('root'), p('bias'), be.ptr(ws), wb, be.stream),
                 'bwd (%s)' % ('overwrite' if overwrite else 'accumulate'))
        return {k: np.asarray(be.get(b)) for k, b in buf.items()}


def same(got, want, what):
    np.testing.assert_array_equal(got, want, err_msg=what)


def check_layer(be, c, relu, bias=True, flags=0):
    """Forward, then the backward twice: overwrite mode -- on the forward's mask words and no `out` where the library
    takes that (register-operand kernels), else on `out` -- and accumulate mode on `out` and no words."""
    ref = c.reference(relu, bias)
    assert ref['bound'] < 2 ** 24            # every sum below is exact in float32, in any order
    d = Device(be, c)
    assert d.flags() == flags
    out, mw = d.forward(relu, bias=bias)
    same(be.get(out), ref['out'], 'out')
    if relu and c.Dout % 64 == 0:
        assert mw is not None
        same(d.mask_bits(mw), ref['out'] > 0, 'mask words')
    want = ALL if bias else ALL[:3]
    no_out = mw is not None and c.Din % 64 == 0
    got = d.backward(relu, 1, want, out=None if no_out or not relu else out, words=mw)
    for k in got:
        same(got[k], ref[k], 'grad_%s (overwrite)' % k)
    got = d.backward(relu, 0, want, out=out if relu else None)
    for k in got:
        same(got[k], ref[k] + (0 if k == 'x' else c.init[k].astype(np.int64)), 'grad_%s (accumulate)' % k)
    assert set(got) == set(want) - ({'basis'} if c.R == 0 else set())
    return d


# ------------------------------------------------------------------------------------------ A: tiles, degenerate shapes
def tile_graph(dims):
    """per-relation edge counts at the 64-row tile edge, one relation with a single edge and one with none; 65 nodes: the
    root pseudo-relation has two tiles, the last of one row"""
    return cached(('tiles', dims), lambda: Case(65, 6, *graph_by_counts([64, 0, 65, 1, 63, 128], 65, 5), dims=dims, seed=41))


def shape_case(shape, dims):
    def make():
        if shape == 'tiles':
            return tile_graph(dims)
        if shape == 'root_513':         # the root has 9 tiles and 2 K chunks, the second of one slot
            return Case(513, 2, *graph_by_counts([37, 63], 513, 6), dims=dims, seed=42)
        if shape == 'one_node':         # only duplicates of the self loop 0 -> 0
            z = np.zeros(70, np.int64)
            return Case(1, 2, z, z, np.random.RandomState(7).randint(0, 2, size=70), dims=dims, seed=43)
        if shape == 'no_edges':         # out = act(bias + x.root); grad_basis zeros / unchanged
            return Case(5, 3, [], [], [], dims=dims, seed=44)
        assert shape == 'no_relations'  # basis = NULL, grad_basis = NULL
        return Case(3, 0, [], [], [], dims=dims, seed=45)
    return cached((shape, dims), make)


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('dims', DIMS, ids=dims_id)
@pytest.mark.parametrize('shape', ['tiles', 'root_513', 'one_node', 'no_edges', 'no_relations'])
def test_tile_edges_and_degenerate_shapes(be, shape, dims, relu):
    c = shape_case(shape, dims)
    if shape == 'tiles':
        assert c.tiles() == 1 + 0 + 2 + 1 + 1 + 2 + 2 and c.Nn % GT_BM == 1
    if shape == 'root_513':
        assert c.slabs()[-1] == 2 and c.Nn % GEN_CHUNK == 1 and c.Nn % GT_BM == 1
    check_layer(be, c, relu)
    if shape == 'no_edges':             # (what the equalities above came to for the relation matrices)
        assert not c.reference(relu)['basis'].any()


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('dims', DIMS, ids=dims_id)
def test_without_bias(be, dims, relu):
    """bias = NULL in the forward, grad_bias = NULL in the backward, on the tile-edge graph"""
    check_layer(be, tile_graph(dims), relu, bias=False)


# ------------------------------------------------------------------------------------------ B: chunk and slab counts
SLAB_COUNTS = [1, 513, 2049, 8193, 0, 8192]


def slab_case(dims):
    return cached(('slabs', dims), lambda: Case(96, 6, *graph_by_counts(SLAB_COUNTS, 96, 8), dims=dims, seed=46))


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('dims', DIMS, ids=dims_id)
def test_slab_counts(be, dims, relu):
    """Relations of 1, 2, 5, 17, 0 and 16 K-chunk slabs through rgcn_gen_reduce_w_kernel -- every request of a trip, the
    clamp of an absent one, the second trip at 17 -- with the last chunk of one slot: (64, 64) the register weight gradient
    and the 16-byte reduction, (40, 24) the LDS-staged K loop and the 16-byte reduction, (5, 3) the scalar reduction with
    its `idx + k < elems` tail. All three dims run on both backends: the 19 000 slots at 64 x 64 take the emulator 6 s,
    under the 10 s at which that one would have gone to the GPU alone."""
    c = slab_case(dims)
    assert c.slabs() == [1, 2, 5, 17, 0, 16, 1]
    check_layer(be, c, relu)


# ------------------------------------------------------------------------------------------ C: column blocks, persistent walk
#            (Din, Dout)  edges per relation      what the side with >= 17 items runs
WALKS = [((64, 64), [2487, 0, 1010, 503]),      # forward and transposed: cb = 1, four row tiles per workgroup
         ((64, 128), [1201, 0, 499, 250]),      # forward: cb = 2, two row tiles per workgroup
         ((192, 64), [560, 0, 230, 110]),       # transposed: cb = 3, the fourth wave leaves
         ((64, 256), [560, 0, 230, 110]),       # forward: cb = 4, one column group
         ((64, 512), [560, 0, 230, 110]),       # forward: cb = 8, two column groups; transposed: 8 mask words per row
         ((512, 64), [560, 0, 230, 110])]       # transposed: cb = 8, two column groups
WALK_NODES = 200


def _items(tiles, cols):
    """(row-tile items, column groups) of rgcn_gen_gemm_rows_kernel for `cols` output columns"""
    cb = cols // 64
    rt = 1 if cb >= 3 else 4 // cb
    return (tiles + rt - 1) // rt, (cb + 3) // 4 if cb >= 4 else 1


@pytest.mark.parametrize('slots', [None, 'few'])
@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('walk', WALKS, ids=lambda w: dims_id(w[0]))
def test_column_blocks_and_persistent_walk(be, walk, relu, slots, request):
    """Every column-block form of the register-operand gather-GEMM, forward and transposed, once on the grid of one
    workgroup per item and once on a GEN_SLOTS grid of 8 workgroups per column group: at least 17 row-tile items on the
    side under test, so a workgroup walks three items and the last trip is partly empty."""
    dims, counts = walk
    c = cached(('walk', dims), lambda: Case(WALK_NODES, 4, *graph_by_counts(counts, WALK_NODES, 9), dims=dims, seed=47))
    sides = [_items(c.tiles(), dims[1]), _items(c.tiles(), dims[0])]
    assert max(n for n, _ in sides) >= 17
    if slots is not None:
        gen = 8 * max(cg for _, cg in sides)
        be.lib.mpqe_debug_option(b'GEN_SLOTS', gen, 1)         # (process-global)
        request.addfinalizer(lambda: be.lib.mpqe_debug_option(b'GEN_SLOTS', 0, 0))
        # the host's grid rule: whole groups of 8 items x column groups, `gen` rounded down to such groups
        trips = [-(-((n + 7) // 8 * 8 * cg) // (gen // (8 * cg) * (8 * cg))) for n, cg in sides]
        assert max(trips) == 3
    check_layer(be, c, relu)


# ------------------------------------------------------------------------------------------ D: wanted outputs only
SUBSETS = [('x',), ('basis', 'root'), ('root',), ('bias',), ('x', 'basis', 'root')]


@pytest.mark.parametrize('source,dims', [('words', (64, 64)), ('out', (64, 64)), ('out', (40, 24))],
                         ids=['words_64x64', 'out_64x64', 'out_40x24'])
def test_wanted_outputs_only(be, source, dims):
    """What autograd asks for (mpqe_amd/ops.py): NULL for every gradient output it does not need. relu = 1, overwrite mode;
    the mask comes from the forward's words with out = NULL, or from `out` with no words (then a bias pass runs only to make
    them when grad_bias is not wanted, and the reduction skips a NULL matrix)."""
    c = tile_graph(dims)
    ref = c.reference(1)
    assert ref['bound'] < 2 ** 24
    d = Device(be, c)
    out, mw = d.forward(1, words=source == 'words')
    assert (mw is not None) == (source == 'words')
    same(be.get(out), ref['out'], 'out')
    src = dict(out=None, words=mw) if source == 'words' else dict(out=out, words=None)
    for want in (ALL,) + tuple(SUBSETS):
        got = d.backward(1, 1, want, **src)
        assert set(got) == set(want)
        for k in want:
            same(got[k], ref[k], 'grad_%s of %s' % (k, '+'.join(want)))


# ------------------------------------------------------------------------------------------ E: many relations
@pytest.mark.parametrize('relu', [0, 1])
def test_many_relations_pointer_tables_in_global_memory(be, relu):
    """R = 2200: R + 2 > 1026 -- the gather-GEMMs read their pointer tables from global memory -- and 2 (R + 2) > 4352 --
    so does the register weight gradient. Edges on six relations around those two limits, 70 each (two tiles, the second
    of 6 rows); every other relation's gradient matrix is zeros in overwrite mode and unchanged in accumulate mode.
    (The 2 200 x 16 idle workgroups of the reduction take the emulator 2 s: it runs there too.)"""
    R, Nn, used = 2200, 70, [0, 1024, 1025, 2173, 2174, 2199]

    def make():
        rng = np.random.RandomState(10)
        typ = rng.permutation(np.repeat(used, 70))
        return Case(Nn, R, rng.randint(0, Nn, size=typ.size), rng.randint(0, Nn, size=typ.size), typ, dims=(64, 64), seed=48)
    c = make()          # (not kept: 36 MB per matrix stack, and its oracle takes 0.2 s)
    assert R + 2 > 1026 and 2 * (R + 2) > 64 * 68
    check_layer(be, c, relu)
    empty = np.setdiff1d(np.arange(R), used)
    assert not c.reference(relu)['basis'][empty].any()


# ------------------------------------------------------------------------------------------ F: clamped indices
@pytest.mark.parametrize('dims', [(8, 8), (64, 64)], ids=dims_id)
def test_bad_indices_are_clamped_to_node_and_relation_zero(be, dims):
    """plan_prep_kernel's documented rule: an endpoint outside [0, Nn) becomes node 0 (each endpoint on its own), a type
    outside [0, R) relation 0, and the flag says so. The layer then computes exactly the layer of that graph."""
    Nn, R = 5, 3

    def make():
        rng = np.random.RandomState(12)
        src, dst, typ = rng.randint(0, Nn, size=40), rng.randint(0, Nn, size=40), rng.randint(0, R, size=40)
        src[:3], dst[:3], typ[:3] = [0, 1, 9], [1, -1, 2], [0, 7, 1]         # test_general_plan_flags_bad_indices' edges
        src[[11, 17]], dst[[17, 23]], typ[[23, 29, 31]] = [-3, Nn], [2 ** 40, Nn], [R, -1, -2 ** 33]
        bad = (src.copy(), dst.copy(), typ.copy())
        src[(src < 0) | (src >= Nn)] = 0
        dst[(dst < 0) | (dst >= Nn)] = 0
        typ[(typ < 0) | (typ >= R)] = 0
        return Case(Nn, R, src, dst, typ, dims=dims, seed=49, bad=bad)
    c = cached(('bad', dims), make)
    assert sum(int((a != b).sum()) for a, b in zip(c.given, (c.src, c.dst, c.typ))) == 3 + 3 + 4
    for relu in (0, 1):
        check_layer(be, c, relu, flags=FLAG_BAD_EDGE | FLAG_BAD_RELATION)
