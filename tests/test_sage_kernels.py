"""mpqe_sage_fwd / mpqe_sage_bwd (csrc/sage.hip) through the C ABI with GIVEN neighbour arrays, on the host emulator and (gpu)
on the real library, against the float64 oracle of tests/sage_oracle.py, and pinned to the reference itself through the two
fixtures tests/golden/sage_depth1_*.npz (the reference's outputs and gradients; its `random` draws are replayed on the host).

Tolerances: `close` of tests/test_op_edges.py -- forward rtol 1e-5, backward rtol 1e-4, atol 2e-6 x the operand scale
max(1, max |ref|); the fixtures at tests/test_model_gpu.py's FWD / BWD (1e-5 / 1e-6 and 1e-4 / 1e-6).

ReLU / LayerNorm kink: an fp32 value on the other side of 0 than its float64 reference flips a mask, and a gradient with it.
The cases' seeds were chosen so that under the ORACLE no value the ReLU sees lies within 1e-4 x its row's largest magnitude of
0; Case asserts that for every element, none left out.

Every operand sits between fences (tests/fenced.py: NaNs for floats); gamma, beta, counts and their gradients 4 bytes off a
16-byte boundary, neigh and self_rows 8 bytes off one (the header demands 16 bytes of the tables, W, out, grad_out and the
gradient buffers); unused neighbour slots hold a huge row, not -1; the workspace is exactly mpqe_sage_workspace_bytes, fenced
and filled with noise; the gradient buffers start non-zero (the call adds)."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

from mpqe_amd import _capi
from tests import sage_oracle as oracle
from tests import test_kg_kernels as K
from tests.fenced import assert_fence_intact, fenced, fenced_bytes
from tests.test_op_edges import close

be = K.be
OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
BAD_INDEX = _capi.FLAG_BAD_INDEX
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FWD = dict(rtol=1e-5, atol=1e-6)
BWD = dict(rtol=1e-4, atol=1e-6)
KINK = 1e-4
UNUSED = 10 ** 12               # what an unused neighbour slot holds here: never read

# (dim_in, dim_out, B, R, max_keep, layer norm, seed): the seed is the first from 0 whose case passes _case's kink check
CASES = {
    'one_row': (16, 16, 1, 1, 1, False, 0),
    'ln_15': (48, 32, 15, 2, 10, True, 0),
    'wide_64': (32, 80, 64, 5, 32, False, 0),
    'ln_65': (32, 80, 65, 2, 10, True, 3),
    'ln_130': (48, 32, 130, 5, 10, True, 3),
    'big_ln_15': (256, 256, 15, 1, 2, True, 6),
    'big_65': (256, 256, 65, 2, 10, False, 82),
}


class Case(object):
    """Inputs of one call in float32 / ints on the host, and the oracle's results. Two tables; block r reads table r % 2, so
    with R >= 2 two relation blocks share a table, and the self block shares one with a relation block. Pad rows: the last
    row of each table."""

    def __init__(self, din, dout, B, R, mk, ln, seed, check_kink=True):
        rng = np.random.RandomState(1000 * seed + din + dout + B)
        self.din, self.dout, self.B, self.R, self.mk, self.ln = din, dout, B, R, mk, ln
        self.K = (R + 1) * din
        self.tables = [rng.randn(n, din).astype(np.float32) for n in (37, 53)]
        self.block_table = np.array([r % 2 for r in range(R + 1)], dtype=np.int32)
        self.block_pad = np.array([self.tables[t].shape[0] - 1 for t in self.block_table], dtype=np.int64)
        counts = rng.randint(0, mk + 1, size=(R, B)).astype(np.int32)
        counts[0] = np.maximum(counts[0], 1)                # block 0: every node has a neighbour, the first one shared
        counts[R - 1, 0] = 0 if R > 1 else counts[R - 1, 0]
        counts[0, B - 1] = mk
        if B > 2:
            counts[R - 1, 1], counts[0, 2] = 0, 1
        neigh = np.full((R, B, mk), UNUSED, dtype=np.int64)
        for r in range(R):
            n = self.tables[self.block_table[r]].shape[0]
            for b in range(B):
                neigh[r, b, :counts[r, b]] = rng.randint(0, n, size=counts[r, b])
        neigh[0, :, 0] = 3                                  # a gradient row with B entries
        self.counts, self.neigh = counts, neigh
        self.self_rows = rng.randint(0, self.tables[self.block_table[R]].shape[0], size=B).astype(np.int64)
        self.self_rows[::7] = -1                            # null nodes
        self.W = (rng.randn(dout, self.K) / np.sqrt(self.K)).astype(np.float32)
        self.gamma = (1.0 + 0.3 * rng.randn(dout)).astype(np.float32) if ln else None
        self.beta = (0.3 * rng.randn(dout)).astype(np.float32) if ln else None
        self.eps = 1e-6
        self.grad_out = rng.randn(B, dout).astype(np.float32)
        self.init = {'tables': [0.5 * rng.randn(*t.shape).astype(np.float32) for t in self.tables],
                     'W': 0.5 * rng.randn(dout, self.K).astype(np.float32), 'gamma': rng.randn(dout).astype(np.float32),
                     'beta': rng.randn(dout).astype(np.float32)}
        eps32 = float(np.float32(self.eps))
        args = (self.tables, self.block_table, self.block_pad, neigh, counts, self.self_rows, self.W)
        self.st = oracle.forward(*args, gamma=self.gamma, beta=self.beta, eps=eps32)
        self.grads = oracle.backward(*args, self.grad_out, gamma=self.gamma, beta=self.beta, eps=eps32, st=self.st)
        pre = self.st['pre']
        self.kink_ok = bool((np.abs(pre) >= KINK * np.abs(pre).max(axis=1, keepdims=True)).all())
        if check_kink:
            assert self.kink_ok, 'a value within %g x its row scale of the ReLU kink: choose another seed' % KINK


@pytest.fixture(scope='module')
def cases():
    """the oracle's results, computed once and shared (nothing changes them)"""
    return {name: Case(*spec) for name, spec in CASES.items()}


class Call(object):
    """One placement of a case's operands on a backend: everything fenced, ready for forward and backward"""

    def __init__(self, be, c, ws_fill='noise', ws_short=0, want=('tables', 'W', 'gamma', 'beta')):
        self.be, self.c = be, c
        T = len(c.tables)
        self.tables = [fenced(be, t) for t in c.tables]
        self.W = fenced(be, c.W)
        self.gamma = fenced(be, c.gamma, misalign=1) if c.ln else None
        self.beta = fenced(be, c.beta, misalign=1) if c.ln else None
        self.neigh = K._at(be, c.neigh, 8) if c.R else None
        self.counts = fenced(be, c.counts, misalign=1) if c.R else None
        self.self_rows = K._at(be, c.self_rows, 8)
        self.out = fenced(be, np.full((c.B, c.dout), np.nan, dtype=np.float32))
        self.grad_out = fenced(be, c.grad_out)
        self.g_tables = [fenced(be, g) if 'tables' in want else None for g in c.init['tables']]
        self.g_W = fenced(be, c.init['W']) if 'W' in want else None
        self.g_gamma = fenced(be, c.init['gamma'], misalign=1) if c.ln and 'gamma' in want else None
        self.g_beta = fenced(be, c.init['beta'], misalign=1) if c.ln and 'beta' in want else None
        self.need = be.lib.mpqe_sage_workspace_bytes(c.B, c.R, c.din, c.dout, c.mk)
        assert self.need >= 256 and self.need % 256 == 0
        self.ws_bytes = self.need - ws_short
        self.ws = fenced_bytes(be, self.ws_bytes, ws_fill, align=256)
        self.err = be.zeros((1,), np.int32)
        self.t_ptrs = (ctypes.c_void_p * T)(*[be.ptr(t) for t in self.tables])
        self.t_rows = (ctypes.c_int64 * T)(*[t.shape[0] for t in c.tables])
        self.g_ptrs = (ctypes.c_void_p * T)(*[be.ptr(g) for g in self.g_tables])

    def _head(self):
        be, c = self.be, self.c
        return (self.t_ptrs, self.t_rows, len(c.tables), c.block_table.ctypes.data, c.block_pad.ctypes.data, c.R,
                be.ptr(self.neigh), be.ptr(self.counts), c.mk, be.ptr(self.self_rows), c.B, be.ptr(self.W), c.din, c.dout,
                be.ptr(self.gamma), be.ptr(self.beta), c.eps)

    def fwd(self, save=1):
        be = self.be
        return be.lib.mpqe_sage_fwd(*(self._head() + (save, be.ptr(self.out), be.ptr(self.ws), self.ws_bytes, be.ptr(self.err),
                                                      be.stream)))

    def bwd(self):
        be = self.be
        return be.lib.mpqe_sage_bwd(*(self._head() + (be.ptr(self.out), be.ptr(self.grad_out), self.g_ptrs, be.ptr(self.g_W),
                                                      be.ptr(self.g_gamma), be.ptr(self.g_beta), be.ptr(self.ws), self.ws_bytes,
                                                      be.ptr(self.err), be.stream)))

    def fences(self):
        be = self.be
        views = self.tables + [self.W, self.gamma, self.beta, self.counts, self.out, self.grad_out, self.g_W, self.g_gamma,
                               self.g_beta, self.ws] + self.g_tables
        for i, v in enumerate(views):
            if v is not None:
                assert_fence_intact(be, v, 'operand %d' % i)

    def results(self):
        """-> dict of host arrays: out and the gradient buffers as they stand"""
        be = self.be
        got = {'out': be.get(self.out), 'err': int(be.get(self.err)[0])}
        for name, v in (('W', self.g_W), ('gamma', self.g_gamma), ('beta', self.g_beta)):
            got[name] = None if v is None else be.get(v)
        got['tables'] = [None if g is None else be.get(g) for g in self.g_tables]
        return got


def _compare(c, got, what):
    close(got['out'], c.st['out'], what=what + ' out')
    g_tables, g_W, g_gamma, g_beta = c.grads
    for t, g in enumerate(got['tables']):
        if g is not None:
            close(g.astype(np.float64) - c.init['tables'][t], g_tables[t], rtol=1e-4, what='%s grad table %d' % (what, t))
    if got['W'] is not None:
        close(got['W'].astype(np.float64) - c.init['W'], g_W, rtol=1e-4, what=what + ' grad W')
    if got['gamma'] is not None:
        close(got['gamma'].astype(np.float64) - c.init['gamma'], g_gamma, rtol=1e-4, what=what + ' grad gamma')
    if got['beta'] is not None:
        close(got['beta'].astype(np.float64) - c.init['beta'], g_beta, rtol=1e-4, what=what + ' grad beta')


# ---------------------------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize('name', list(CASES))
def test_forward_and_backward_against_the_oracle(be, cases, name):
    """Forward, then backward, every operand fenced, the workspace exact and full of noise; the pad rows, the row every node
    shares and the rows two blocks reach through one table are among the gradient rows compared."""
    c = cases[name]
    call = Call(be, c)
    assert call.fwd() == OK
    assert call.bwd() == OK
    call.fences()
    got = call.results()
    assert got['err'] == 0
    _compare(c, got, name)
    g_tables = c.grads[0]
    assert np.abs(g_tables[0][3]).max() > 0 and np.abs(g_tables[c.block_table[c.R]][-1]).max() > 0      # shared row, a pad row
    for view, host in ((call.W, c.W), (call.grad_out, c.grad_out), (call.counts, c.counts), (call.tables[0], c.tables[0])):
        np.testing.assert_array_equal(be.get(view), host)                      # inputs are read only
    # inference: no states, no workspace -- the same output bits
    bare = Call(be, c)
    bare.ws = None
    assert bare.fwd(save=0) == OK
    np.testing.assert_array_equal(bare.results()['out'], got['out'])


def test_the_same_call_twice_gives_the_same_bits(be, cases):
    c = cases['ln_130']
    runs = []
    for fill in ('noise', 'nan'):
        call = Call(be, c, ws_fill=fill)
        assert call.fwd() == OK and call.bwd() == OK
        runs.append(call.results())
    for key in ('out', 'W', 'gamma', 'beta'):
        np.testing.assert_array_equal(runs[0][key], runs[1][key], err_msg=key)
    for a, b in zip(runs[0]['tables'], runs[1]['tables']):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize('want', [('W',), ('tables',), ('gamma', 'beta'), ()])
def test_null_gradient_pointers_are_skipped(be, cases, want):
    c = cases['ln_15']
    call = Call(be, c, want=want)
    assert call.fwd() == OK and call.bwd() == OK
    call.fences()
    _compare(c, call.results(), 'only %s' % (want,))


def test_workspace_one_byte_short_is_refused(be, cases):
    c = cases['ln_15']
    call = Call(be, c, ws_short=1)
    before = be.get(call.out).copy()
    assert call.fwd() == WORKSPACE and call.bwd() == WORKSPACE
    np.testing.assert_array_equal(be.get(call.out), before)                    # nothing ran
    np.testing.assert_array_equal(be.get(call.g_W), c.init['W'])
    call.fences()
    assert call.fwd(save=0) == OK                                              # inference does not need it


def test_out_of_range_rows_are_flagged_and_read_as_zeros(be):
    """A neighbour row at its table's row count, a negative row in a used slot, a self row beyond its table and a count above
    max_keep: MPQE_FLAG_BAD_INDEX; the oracle reads such rows as zeros, takes that count as 0 (the pad row), and gives them no
    gradient -- the rest agrees."""
    c = Case(32, 80, 20, 2, 10, True, 1, check_kink=False)
    c.counts[0, 4], c.counts[1, 5], c.counts[1, 6] = 3, 2, 11
    c.neigh[0, 4, 1], c.neigh[1, 5, 0] = 37, -1
    c.self_rows[9] = 53
    call = Call(be, c)
    shown = c.counts.copy()
    c.counts[1, 6] = 0                                                         # what the kernels make of it
    eps32 = float(np.float32(c.eps))
    args = (c.tables, c.block_table, c.block_pad, c.neigh, c.counts, c.self_rows, c.W)
    c.st = oracle.forward(*args, gamma=c.gamma, beta=c.beta, eps=eps32)
    c.grads = oracle.backward(*args, c.grad_out, gamma=c.gamma, beta=c.beta, eps=eps32, st=c.st)
    pre = c.st['pre']
    assert (np.abs(pre) >= KINK * np.abs(pre).max(axis=1, keepdims=True)).all()
    np.testing.assert_array_equal(be.get(call.counts), shown)
    assert call.fwd() == OK and call.bwd() == OK
    call.fences()
    got = call.results()
    assert got['err'] == BAD_INDEX
    _compare(c, got, 'bad rows')


# ---------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize('name', ['sage_depth1_plain', 'sage_depth1_ln'])
def test_pinned_to_the_reference(be, name):
    """The reference's draws replayed on the host exactly as mpqe_amd/aggregators.py makes them (random.seed, relations in
    order, one random.sample per node, the sample as a set), turned into neigh / counts; `out` and every gradient against
    what the reference produced."""
    z = np.load(os.path.join(GOLDEN, name + '.npz'))
    meta = json.loads(bytes(z['meta']).decode())
    modes, mode, D = meta['schema']['modes'], meta['mode'], meta['D']
    rels = [tuple(x) for x in meta['schema']['relations'][mode]]
    adj = {tuple(rel): {int(n): list(nb) for n, nb in items} for rel, items in meta['adj']}
    node_map, nodes = z['node_map'], z['nodes'].tolist()
    R, B, mk = len(rels), len(nodes), meta['max_keep']
    random.seed(meta['random_seed'])
    neigh = np.full((R, B, mk), -1, dtype=np.int64)
    counts = np.zeros((R, B), dtype=np.int32)
    for r, (to_mode, rel_name) in enumerate(rels):
        lists = adj[(mode, rel_name, to_mode)]
        for b, n in enumerate(nodes):
            nb = lists[n]
            picks = set(random.sample(nb, min(int(np.ceil(len(nb) * meta['keep_prob'])), mk)))
            neigh[r, b, :len(picks)] = node_map[list(picks)]
            counts[r, b] = len(picks)
    c = Case.__new__(Case)
    c.din = c.dout = D
    c.B, c.R, c.mk, c.ln, c.K, c.eps = B, R, mk, meta['layer_norm'], (R + 1) * D, 1e-6
    c.tables = [z['param/feat-%s.weight' % m] for m in modes]
    c.block_table = np.array([modes.index(t) for t, _ in rels] + [modes.index(mode)], dtype=np.int32)
    c.block_pad = np.array([c.tables[t].shape[0] - 1 for t in c.block_table], dtype=np.int64)
    c.neigh, c.counts, c.self_rows = neigh, counts, node_map[nodes].astype(np.int64)
    c.W = z['param/%s_compress' % mode]
    c.gamma = z['param/%s_ln.gamma' % mode] if c.ln else None
    c.beta = z['param/%s_ln.beta' % mode] if c.ln else None
    c.grad_out = np.ascontiguousarray(z['grad_out'].T)
    c.init = {'tables': [np.zeros_like(t) for t in c.tables], 'W': np.zeros_like(c.W),
              'gamma': np.zeros(D, dtype=np.float32), 'beta': np.zeros(D, dtype=np.float32)}
    call = Call(be, c)
    assert call.fwd() == OK and call.bwd() == OK
    call.fences()
    got = call.results()
    assert got['err'] == 0
    np.testing.assert_allclose(got['out'].T, z['out'], **FWD)
    np.testing.assert_allclose(got['W'], z['grad/%s_compress' % mode], err_msg='compress', **BWD)
    for t, m in enumerate(modes):
        np.testing.assert_allclose(got['tables'][t], z['grad/feat-%s.weight' % m], err_msg=m, **BWD)
    if c.ln:
        np.testing.assert_allclose(got['gamma'], z['grad/%s_ln.gamma' % mode], **BWD)
        np.testing.assert_allclose(got['beta'], z['grad/%s_ln.beta' % mode], **BWD)


# ---------------------------------------------------------------------------------------------- refused before launch
@pytest.mark.parametrize('which', ['emu', 'product'])
def test_refused_before_any_launch(which):
    """Device pointers are made-up addresses: a call that launched anything with them would fault."""
    from tests.test_kg_sample_kernels import _libs
    lib = _libs()[which]()
    fake = 0x10000
    tabs, rows = (ctypes.c_void_p * 2)(fake, fake), (ctypes.c_int64 * 2)(30, 40)

    def fwd(tables=tabs, T=2, bt=(0, 1, 0), pad=(29, 39, 29), R=2, neigh=fake, counts=fake, mk=10, self_rows=fake, B=5, W=fake,
            din=32, dout=48, gamma=fake, beta=fake, save=1, out=fake, ws=fake, wb=1 << 30):
        bt_, pad_ = np.asarray(bt, dtype=np.int32), np.asarray(pad, dtype=np.int64)
        return lib.mpqe_sage_fwd(tables, rows, T, bt_.ctypes.data, pad_.ctypes.data, R, neigh, counts, mk, self_rows, B, W, din,
                                 dout, gamma, beta, 1e-6, save, out, ws, wb, None, None)
    size = lib.mpqe_sage_workspace_bytes
    need = size(5, 2, 32, 48, 10)
    assert need >= 256 and need % 256 == 0
    assert size(5, 2, 24, 48, 10) == 0 and size(5, 2, 32, 272, 10) == 0 and size(5, 2, 0, 48, 10) == 0
    assert size(-1, 2, 32, 48, 10) == 0 and size(5, 65, 32, 48, 10) == 0 and size(5, 2, 32, 48, 0) == 0 and size(5, 2, 32, 48, 33) == 0
    assert size(1 << 24, 64, 32, 48, 32) == 0                                  # 2^31 entries and more
    assert fwd(din=24) == UNSUPPORTED and fwd(dout=8) == UNSUPPORTED and fwd(din=272) == UNSUPPORTED
    assert fwd(mk=0) == INVALID and fwd(mk=33) == INVALID and fwd(R=65) == INVALID and fwd(B=-1) == INVALID
    assert fwd(tables=None) == INVALID and fwd(T=0) == INVALID and fwd(bt=(0, 2, 0)) == INVALID and fwd(pad=(29, 40, 29)) == INVALID
    assert fwd(pad=(-1, 39, 29)) == INVALID and fwd(tables=(ctypes.c_void_p * 2)(fake, fake + 4)) == INVALID
    assert fwd(W=None) == INVALID and fwd(W=fake + 4) == INVALID and fwd(gamma=None) == INVALID and fwd(beta=None) == INVALID
    assert fwd(neigh=None) == INVALID and fwd(counts=None) == INVALID and fwd(self_rows=None) == INVALID
    assert fwd(out=None) == INVALID and fwd(out=fake + 8) == INVALID
    assert fwd(ws=None) == INVALID and fwd(ws=fake + 16) == INVALID and fwd(wb=need - 1) == WORKSPACE
    assert fwd(B=0) == OK and fwd(B=0, neigh=None, counts=None, self_rows=None, out=None) == OK

    def bwd(out=fake, gout=fake, gt=tabs, gW=fake, ws=fake, wb=1 << 30, B=5):
        bt_, pad_ = np.array([0, 1, 0], dtype=np.int32), np.array([29, 39, 29], dtype=np.int64)
        return lib.mpqe_sage_bwd(tabs, rows, 2, bt_.ctypes.data, pad_.ctypes.data, 2, fake, fake, 10, fake, B, fake, 32, 48,
                                 fake, fake, 1e-6, out, gout, gt, gW, fake, fake, ws, wb, None, None)
    assert bwd(out=None) == INVALID and bwd(gout=None) == INVALID and bwd(gout=fake + 4) == INVALID
    assert bwd(gW=fake + 4) == INVALID and bwd(gt=(ctypes.c_void_p * 2)(fake, fake + 4)) == INVALID
    assert bwd(ws=None) == INVALID and bwd(wb=need - 1) == WORKSPACE and bwd(B=0) == OK
