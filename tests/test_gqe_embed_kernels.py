"""mpqe_gqe_embed (csrc/gqe.hip): the rows a GQE programme scores, through the C ABI against the float64 oracle
(tests/gqe_oracle.py), on the host emulator and on the GPU (the parametrisation of tests/test_gqe_kernels.py).

The scored P-side rows are on the oracle's tape after Oracle.forward: in a chain formula the first parent of the final
`cos` node, in an intersection formula the row set its `take` draws from.
Tolerance: the project's forward tolerance (gqe_oracle.FWD: rtol 1e-5, atol 1e-6) per element against the row's largest
magnitude, |got - want| <= 1e-6 + 1e-5 max|want_row|. Every problem is the first seed for which the oracle alone finds no
near-tie, the problem well conditioned (gqe_common.settled_problem's two conditions) and, the same idea applied to the
rows, the oracle's own op sequence in float32 within HALF of that bound of the float64 rows. Nothing is dropped; the
search (at most 50 seeds) runs on the CPU and reads the oracle alone.
Shapes: those of tests/test_gqe_kernels.py -- D 16 / 48 / 128 at B 1 / 17 / 33, D 64 / 80 / 256 at B 17; an intersection
formula's P rows are its B queries, a chain formula's its B targets and ragged negatives (gqe_common.NEG_CYCLE, duplicate
ids). Identity mode (p_ids = NULL): 23 rows of the 24-row table, two workgroups with a 7-row tail, 16 guard rows behind."""
import argparse
import ctypes

import numpy as np
import pytest

from tests import gqe_common as gc
from tests.gqe_oracle import FWD, Oracle

TYPES = ['1-chain', '2-chain', '3-chain', '2-inter', '3-inter', '3-inter_chain', '3-chain_inter']
OK, INVALID, UNSUPPORTED = 0, -1, -2
SENTINEL = -7.5


@pytest.fixture(scope='module', params=['emu', pytest.param('hip', marks=pytest.mark.gpu)])
def be(request):
    from tests import kernel_backend
    if request.param == 'emu':
        return kernel_backend.EmuBackend()
    return kernel_backend.HipBackend()


def row_bound(want):
    return FWD['atol'] + FWD['rtol'] * np.abs(want).max(axis=1, keepdims=True)


def scored_rows(o, chain):
    """The P-side rows the last Oracle.forward scored."""
    parents = {id(node): ps for node, ps, _ in o.tape}
    a, b = parents[id(o.out)]
    if chain:
        return a.v                      # cos(projected target / negative rows, take(anchor embeddings))
    (q,) = parents[id(b)]               # cos(target embeddings, take(query rows))
    return q.v


def rows_settle(prob, rows, forward):
    """The oracle's op sequence in float32 stays within half the bound of its float64 rows."""
    o32 = Oracle(prob.params, prob.node_map, dtype=np.float32)
    forward(o32)
    return bool((np.abs(scored_rows(o32, 'inter' not in prob.formula.query_type).astype(np.float64) - rows) <= 0.5 * row_bound(rows)).all())


_SETTLED = {}


def settled(qt, D, B, inter):
    """(problem, oracle rows): computed once, shared by both backends, left unchanged."""
    key = (qt, D, B, inter)
    if key not in _SETTLED:
        seed = 100 * TYPES.index(qt) + D + B
        for s in range(seed, seed + 50):
            prob = gc.Problem(qt, D, B, inter, s)
            o, scores = prob.oracle()
            rows = scored_rows(o, 'inter' not in qt).copy()
            if prob.near_ties(o) == 0 and prob.well_conditioned(o, scores) and rows_settle(
                    prob, rows, lambda o32: o32.forward(prob.formula, prob.anchors, prob.targets, prob.negs,
                                                        prob.neg_lengths, prob.inter)):
                _SETTLED[key] = (prob, rows)
                break
        else:
            raise AssertionError('no settled seed among the 50 tried')
    return _SETTLED[key]


def identity_forward(prob):
    ids = prob.ids[prob.formula.target_mode]
    anchors = np.repeat(prob.anchors[:1], ids.shape[0], axis=0)
    return lambda o: o.forward(prob.formula, anchors, ids, inter=prob.inter)


def settled_identity(qt, D):
    """(problem, oracle rows of the ids that map to rows 0 .. 22 of the target mode's table)."""
    key = (qt, D, 'identity')
    if key not in _SETTLED:
        seed = 100 * TYPES.index(qt) + D
        for s in range(seed, seed + 50):
            prob = gc.Problem(qt, D, 5, 'mean', s)
            assert (prob.node_map[prob.ids[prob.formula.target_mode]] == np.arange(23)).all()
            o = Oracle(prob.params, prob.node_map)
            identity_forward(prob)(o)
            rows = scored_rows(o, True).copy()
            if rows_settle(prob, rows, identity_forward(prob)):
                _SETTLED[key] = (prob, rows)
                break
        else:
            raise AssertionError('no settled seed among the 50 tried')
    return _SETTLED[key]


def embed(be, prob, p_ids='packed', node_map=True, p_rows=None, guard=0, D=None, num_mats=None, out_shift=0, prog=None,
          fake=None):
    """One mpqe_gqe_embed call -> (status, out [p_rows + guard, D] as numpy, error word). fake: an address to pass for every
    device pointer (a call that must be refused before any launch)."""
    pk = gc.pack(prob)
    prog = np.ascontiguousarray(pk[0] if prog is None else prog, dtype=np.int32)
    modes, mat_keys = pk[1], pk[2]
    if isinstance(p_ids, str):
        p_ids = pk[3]
    if p_rows is None:
        p_rows = p_ids.shape[1]
    D = prob.D if D is None else D
    rows = (ctypes.c_int64 * len(modes))(*[prob.params['enc.feat-%s.weight' % m].shape[0] for m in modes])
    nm_len = int(prob.node_map.shape[0]) if node_map else 0
    if fake is not None:
        tab = (ctypes.c_void_p * len(modes))(*[fake] * len(modes))
        mat = (ctypes.c_void_p * max(len(mat_keys), 1))(*[fake] * max(len(mat_keys), 1))
        return be.lib.mpqe_gqe_embed(prog.ctypes.data, tab, rows, len(modes), fake if node_map else None, nm_len, mat,
                                     len(mat_keys) if num_mats is None else num_mats, D, None if p_ids is None else fake,
                                     p_rows, fake + out_shift, None, None), None, None
    tables = [be.put(prob.params['enc.feat-%s.weight' % m]) for m in modes]
    mats = [be.put(prob.params[k]) for k in mat_keys]
    d_map = be.put(prob.node_map) if node_map else None
    d_ids = None if p_ids is None else be.put(np.ascontiguousarray(p_ids, dtype=np.int64))
    out = be.empty((p_rows + guard, D), np.float32, fill=SENTINEL)
    err = be.zeros(1, np.int32)
    tab = (ctypes.c_void_p * len(tables))(*[be.ptr(t) for t in tables])
    mat = (ctypes.c_void_p * max(len(mats), 1))(*[be.ptr(m) for m in mats])
    st = be.lib.mpqe_gqe_embed(prog.ctypes.data, tab, rows, len(tables), be.ptr(d_map), nm_len, mat, len(mats), D,
                               be.ptr(d_ids), p_rows, be.ptr(out), be.ptr(err), be.stream)
    return st, be.get(out), int(be.get(err)[0])


def check_rows(got, want, what=''):
    err = np.abs(got.astype(np.float64) - want)
    print('%s rows: max abs error %.3g (max |ref| %.3g)' % (what, err.max(), np.abs(want).max()))
    assert got.shape == want.shape
    assert (err <= row_bound(want)).all(), 'worst error / bound %.3g' % (err / row_bound(want)).max()


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
def test_rows_against_oracle(be, qt, D, B, inter):
    prob, rows = settled(qt, D, B, inter)
    p_ids = gc.pack(prob)[3]
    if 'inter' in qt:
        assert p_ids.shape[1] == B and rows.shape == (B, D)
    else:
        assert p_ids.shape == (1, prob.n) and rows.shape == (prob.n, D)
        if B > 1:
            assert (prob.neg_lengths == 0).any() and (prob.neg_lengths > 16).any() and prob.targets[B - 1] == prob.targets[0]
    st, got, err = embed(be, prob)
    assert st == OK and err == 0
    check_rows(got, rows, qt)


@pytest.mark.parametrize('qt', ['1-chain', '3-chain'])
@pytest.mark.parametrize('D', [48, 256])
def test_identity_mode(be, qt, D):
    """p_ids = NULL: row r of the table is P row r -- the bits of p_ids = arange without a node_map, the oracle's rows, and
    nothing stored past out + p_rows * dim."""
    prob, rows = settled_identity(qt, D)
    st, got, err = embed(be, prob, p_ids=None, node_map=False, p_rows=23, guard=16)
    assert st == OK and err == 0
    assert (got[23:] == SENTINEL).all(), 'the tail tile stored past the last row'
    st, listed, err = embed(be, prob, p_ids=np.arange(23).reshape(1, 23), node_map=False, guard=16)
    assert st == OK and err == 0
    assert (listed[23:] == SENTINEL).all()
    assert got.tobytes() == listed.tobytes()
    check_rows(got[:23], rows, qt)
    # through the ids and node_map: the same lookups, the same bits
    st, mapped, err = embed(be, prob, p_ids=prob.ids[prob.formula.target_mode].reshape(1, 23))
    assert st == OK and err == 0 and mapped.tobytes() == got[:23].tobytes()


def test_run_to_run_bits(be):
    prob, rows = settled('3-inter_chain', 128, 33, 'min')
    a, b = embed(be, prob), embed(be, prob)
    assert a[0] == OK and b[0] == OK
    assert a[1].tobytes() == b[1].tobytes()
    prob, rows = settled('3-chain', 128, 33, 'mean')
    assert embed(be, prob)[1].tobytes() == embed(be, prob)[1].tobytes()


@pytest.mark.parametrize('qt', ['2-chain', '3-inter'])
def test_bad_id_flags_and_spares_the_other_rows(be, qt):
    prob, rows = settled(qt, 48, 17, 'mean')
    st, want, err = embed(be, prob)
    assert st == OK and err == 0
    p_ids = gc.pack(prob)[3].copy()
    victim = 5
    p_ids[0, victim] = prob.node_map.shape[0] - 1              # (in the map, of no mode: -1)
    st, got, err = embed(be, prob, p_ids=p_ids)
    assert st == OK, 'the call returns'
    assert err & 1
    assert np.isfinite(got).all()
    keep = np.arange(got.shape[0]) != victim
    assert got[keep].tobytes() == want[keep].tobytes()
    if qt == '2-chain':
        assert not got[victim].any(), 'a zero row through the matrices stays zero'


@pytest.mark.parametrize('which', ['emu', 'product'])
def test_refusals_before_any_launch(which):
    """Device pointers are made-up addresses: a call that launched anything with them would fault. Every call here must
    answer from its checks."""
    from mpqe_amd import _lib, ops
    from tests.kernel_backend import EmuBackend

    be = argparse.Namespace(lib=EmuBackend().lib if which == 'emu' else _lib.load())
    fake = 0x10000
    chain = gc.Problem('2-chain', 32, 5, 'mean', 0)
    inter = gc.Problem('2-inter', 32, 5, 'mean', 0)
    assert embed(be, chain, fake=fake, D=24)[0] == UNSUPPORTED
    assert embed(be, chain, fake=fake, D=272)[0] == UNSUPPORTED
    assert embed(be, inter, fake=fake, p_ids=None, p_rows=5)[0] == INVALID          # no id list with two branches
    assert embed(be, chain, fake=fake, p_ids=None, p_rows=25)[0] == INVALID         # the table has 24 rows
    assert embed(be, chain, fake=fake, out_shift=4)[0] == INVALID                   # `out` not 16-byte aligned
    for prob in (chain, inter):                                                     # the programme's last matrix is out of range
        assert embed(be, prob, fake=fake, num_mats=len(gc.pack(prob)[2]) - 1)[0] == INVALID
    assert embed(be, chain, fake=fake, p_rows=0)[0] == INVALID
    bad = np.array(gc.pack(inter)[0])
    bad[1] = 4                                                                      # four branches
    assert embed(be, inter, fake=fake, prog=bad)[0] == INVALID
    assert be.lib.mpqe_gqe_embed(None, None, None, 1, None, 0, None, 0, 32, None, 5, fake, None, None) == INVALID
    assert ops.GQE_PROG_INTS == 32


# ------------------------------------------------------------------ the two operands of answering a query, on the emulator
def tol(s):
    return 2e-6 + 1e-5 * np.abs(s)


def bracket(scores, ids, target, banned=()):
    """lo / hi of the rank of `target` from one query's scores of all entities, widened by 2 tol (tests/test_answer_gpu.py)."""
    st = float(scores[ids == target][0])
    keep = np.array([i != target and i not in banned for i in ids])
    so = scores[keep].astype(np.float64)
    return 1 + int((so > st + 2 * tol(st)).sum()), 1 + int((so >= st - 2 * tol(st)).sum())


@pytest.mark.parametrize('qt,inter', [('2-chain', 'mean'), ('3-inter_chain', 'min')])
def test_embed_then_rank_gives_the_oracle_ranks(qt, inter):
    """What QueryEncoderDecoder.rank_targets does on the fused path, at the C ABI: chain form -- the mode's table projected
    once (identity mode) and the normalised anchors ranked against it; intersection form -- the query rows ranked against
    the raw table. The ranks lie in the bracket of the oracle's scores of every entity."""
    from tests.kernel_backend import EmuBackend
    embed_then_rank(EmuBackend(), qt, inter)


def embed_then_rank(be, qt, inter):
    prob, _ = settled(qt, 48, 17, inter)
    f, B, D, n = prob.formula, prob.B, prob.D, 23
    ids_all = prob.ids[f.target_mode]
    o = Oracle(prob.params, prob.node_map)
    s = o.forward(f, prob.anchors, prob.targets, np.tile(ids_all, B), [n] * B, inter)[B:].reshape(B, n)
    table = prob.params['enc.feat-%s.weight' % f.target_mode]
    err = be.zeros(1, np.int32)
    if 'inter' in qt:
        st, q, e = embed(be, prob)
        cand = np.ascontiguousarray(table[:n])
    else:
        st, cand, e = embed(be, prob, p_ids=None, node_map=False, p_rows=n)
        anchors = be.put(prob.anchors[:, 0].astype(np.int64))
        tab = be.put(prob.params['enc.feat-%s.weight' % f.anchor_modes[0]])
        nm = be.put(prob.node_map)
        q = be.empty((B, D), np.float32)
        assert be.lib.mpqe_embed_l2norm_fwd(be.ptr(tab), tab.shape[0], D, be.ptr(nm), nm.shape[0], be.ptr(anchors), B,
                                            be.ptr(q), D, None, be.ptr(err), be.stream) == OK
        q = be.get(q)
    assert st == OK and e == 0
    target_rows = be.put(prob.node_map[prob.targets])
    dq, dc = be.put(q), be.put(cand)
    rank, tsc = be.empty((B,), np.int64), be.empty((B,), np.float32)
    need = be.lib.mpqe_rank_workspace_bytes(B, n, D, 0)
    ws = be.nbytes(need)
    assert be.lib.mpqe_rank_entities(be.ptr(dq), B, be.ptr(dc), n, D, 1e-8, be.ptr(target_rows), None, None, 0, 0, None, None,
                                     be.ptr(rank), be.ptr(tsc), be.ptr(ws), need, be.ptr(err), be.stream) == OK
    assert int(be.get(err)[0]) == 0
    rank, tsc = be.get(rank), be.get(tsc)
    for i in range(B):
        want = s[i][ids_all == prob.targets[i]][0]
        assert abs(tsc[i] - want) <= tol(want), (i, tsc[i], want)
        lo, hi = bracket(s[i], ids_all, prob.targets[i])
        assert lo <= rank[i] <= hi, (i, rank[i], lo, hi)
