"""mpqe_rank_entities_mixed: the queries of one call ranked against different candidate sets.

Runs on the host fiber emulator (`emu`, no GPU needed) and on the gfx950 library (`hip`, marked gpu).

The oracle is the library's own per-table call on the same backend: every output of query i must equal, to the bit, what
mpqe_rank_entities_scored returns when the queries of i's set are handed to it alone, with the set's score kind and the
exclusion list "rows of the set whose excl_bits bit is set or whose valid bit is clear". One case is also held against
float64 with tests/test_rank.py's tolerance and checkers (imported, not copied); tests/test_rank_exact.py holds the call,
bitmaps included, against an int64 oracle that shares nothing with the library.

The main shape: five sets of 1, 63, 64, 65 and 700 rows, Q = 150 interleaved so that the sets get 0, 1, 64, 65 and 20
queries (an empty set, a one-query block, a full block, a block and a query, a partial block). The block bound is
150 / 64 + 5 = 7, so the strip rule of rank_core.h gives S = 11 strips of one tile for the 700-row set and the narrower sets
leave most strips empty; test_a_wide_set_several_tiles_per_strip widens a set until a strip of it holds two tiles. Operands
sit between NaN fences; the descriptor block and the workspace are exactly as large as the size functions say and hold
garbage.
"""
import ctypes

import numpy as np
import pytest

from mpqe_amd._capi import FLAG_BAD_INDEX
from tests.fenced import assert_fence_intact, fenced, fenced_bytes
from tests.test_rank import check_rank, check_topk, truth

MAX_K = 128
EPS = 1e-8
ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -2, -3
ROWS = (1, 63, 64, 65, 700)
COUNTS = (0, 1, 64, 65, 20)


@pytest.fixture(scope='module', params=['emu', pytest.param('hip', marks=pytest.mark.gpu)])
def be(request):
    from tests import kernel_backend
    if request.param == 'emu':
        return kernel_backend.EmuBackend()
    return kernel_backend.HipBackend()


class Problem(object):
    """Host-side description of one call; build() draws it."""

    def __init__(self, q, tables, kinds, valid, set_of_group, group_of, target, bits):
        self.q, self.tables, self.kinds, self.valid = q, tables, kinds, valid
        self.set_of_group, self.group_of, self.target, self.bits = set_of_group, group_of, target, bits

    def set_of(self, i):
        g = int(self.group_of[i])
        return int(self.set_of_group[g]) if 0 <= g < len(self.set_of_group) else -1

    def excluded(self, i):
        """The sorted exclusion list of query i in rows of its set."""
        s = self.set_of(i)
        n = self.tables[s].shape[0]
        rows = np.arange(n)
        out = np.zeros(n, dtype=bool)
        if self.bits is not None:
            w = self.bits[i].view(np.uint32)
            inside = rows // 32 < w.shape[0]
            out[inside] |= ((w[rows[inside] // 32] >> (rows[inside] % 32).astype(np.uint32)) & 1).astype(bool)
        if self.valid is not None and self.valid[s] is not None:
            v = self.valid[s].view(np.uint32)
            out |= ~((v[rows // 32] >> (rows % 32).astype(np.uint32)) & 1).astype(bool)
        return rows[out].tolist()

    def take(self, idx):
        idx = np.asarray(idx)
        return Problem(self.q[idx], self.tables, self.kinds, self.valid, self.set_of_group, self.group_of[idx],
                       None if self.target is None else self.target[idx], None if self.bits is None else self.bits[idx])


def interleave(counts, rng):
    """Set index per query: every set's queries spread over the whole call, in a fixed random order."""
    sets = np.concatenate([np.full(c, s, dtype=np.int64) for s, c in enumerate(counts)])
    return sets[rng.permutation(sets.shape[0])]


def build(seed, dim, rows=ROWS, counts=COUNTS, kinds=None, with_bits=True, with_valid=True, W=None):
    rng = np.random.RandomState(seed)
    num_sets = len(rows)
    tables = [(rng.randn(n, dim) * (0.5 + rng.rand(n, 1))).astype(np.float32) for n in rows]
    kinds = list(kinds) if kinds is not None else [s % 2 for s in range(num_sets)]      # cosine and dot in one call
    qset = interleave(counts, rng)
    Q = qset.shape[0]
    # two groups per set, numbered so that group order is not set order
    set_of_group = np.array([s for s in range(num_sets)][::-1] + [s for s in range(num_sets)], dtype=np.int32)
    group_of = np.array([(num_sets - 1 - s) if i % 2 else num_sets + s for i, s in enumerate(qset)], dtype=np.int64)
    q = rng.randn(Q, dim).astype(np.float32)
    target = np.array([rng.randint(0, rows[s]) for s in qset], dtype=np.int64)
    bits = None
    if with_bits:
        W = W if W is not None else (max(rows) + 31) // 32 + 2          # wider than the widest set
        dense = rng.rand(Q, W * 32) < 0.2                                # bits beyond every set's rows are set too
        for i in range(Q):
            if i % 3 == 0:
                dense[i, target[i]] = True                               # the target's own bit
            if i % 3 == 1:
                dense[i, target[i]] = False
        dense[:, max(rows):] |= rng.rand(Q, W * 32 - max(rows)) < 0.5
        bits = np.packbits(dense.reshape(Q, W, 32), axis=2, bitorder='little').view('<u4').reshape(Q, W).view(np.int32)
    valid = None
    if with_valid:
        valid = []
        for s, n in enumerate(rows):
            if s % 2 == 0 and n > 1:
                valid.append(None)
                continue
            ok = rng.rand((n + 31) // 32 * 32) < 0.8                    # holes; the words' spare bits are random
            ok[0] = True
            valid.append(np.packbits(ok.reshape(-1, 32), axis=1, bitorder='little').view('<u4').reshape(-1).view(np.int32))
    return Problem(q, tables, kinds, valid, set_of_group, group_of, target, bits)


def run_mixed(be, pb, k, fill='noise', status=0, ws_short=0, want_rank=True, keep=None, mis_q=0):
    """One mixed call on fenced operands with a descriptor block and a workspace of exactly the named sizes; the query
    matrix `mis_q` floats off 16 bytes."""
    lib = be.lib
    Q, D = pb.q.shape
    num_sets, num_groups = len(pb.tables), len(pb.set_of_group)
    rows = np.array([t.shape[0] for t in pb.tables], dtype=np.int64)
    dt = [fenced(be, t) for t in pb.tables]
    dv = [None if (pb.valid is None or v is None) else fenced(be, v) for v in (pb.valid or [None] * num_sets)]
    tabs = (ctypes.c_void_p * num_sets)(*[be.ptr(t) for t in dt])
    vals = (ctypes.c_void_p * num_sets)(*[be.ptr(v) for v in dv])
    kinds = np.array(pb.kinds, dtype=np.int32)
    need_d = lib.mpqe_rank_mixed_desc_bytes(num_sets, num_groups)
    assert need_d > 0
    desc = fenced_bytes(be, need_d, fill)
    st = lib.mpqe_rank_mixed_desc_build(tabs, rows.ctypes.data, kinds.ctypes.data, vals, num_sets,
                                        pb.set_of_group.ctypes.data, num_groups, be.ptr(desc), need_d, be.stream)
    assert st == 0, 'descriptor build: %d' % st
    max_rows, total_rows = int(rows.max()), int(rows.sum())
    dq = fenced(be, pb.q, mis_q)
    dg = fenced(be, pb.group_of)
    dtg = None if pb.target is None else fenced(be, pb.target)
    W = 0 if pb.bits is None else pb.bits.shape[1]
    db = None if pb.bits is None else fenced(be, pb.bits)
    kk = max(k, 1)
    topr = fenced(be, np.full((Q, kk), -7, dtype=np.int64)) if k > 0 else None
    tops = fenced(be, np.full((Q, kk), np.nan, dtype=np.float32)) if k > 0 else None
    ranked = pb.target is not None and want_rank
    rank = fenced(be, np.full((Q,), -7, dtype=np.int64)) if ranked else None
    tsc = fenced(be, np.full((Q,), np.nan, dtype=np.float32)) if ranked else None
    need = lib.mpqe_rank_mixed_workspace_bytes(Q, num_sets, max_rows, total_rows, D, k)
    assert need > 0
    ws = fenced_bytes(be, need, fill)
    err = be.zeros((1,), np.int32)
    st = lib.mpqe_rank_entities_mixed(be.ptr(dq), Q, D, EPS, be.ptr(desc), need_d, num_sets, num_groups, max_rows,
                                      total_rows, be.ptr(dg), be.ptr(dtg), be.ptr(db), W, k, be.ptr(topr), be.ptr(tops),
                                      be.ptr(rank), be.ptr(tsc), be.ptr(ws), need - ws_short, be.ptr(err), be.stream)
    assert st == status, 'status %d, expected %d' % (st, status)
    get = lambda a: None if a is None else be.get(a)
    out = {'rows': get(topr), 'scores': get(tops), 'rank': get(rank), 'tscore': get(tsc), 'err': int(be.get(err)[0])}
    for name, a in [('q', dq), ('group_of', dg), ('targets', dtg), ('bits', db), ('topk rows', topr), ('topk scores', tops),
                    ('rank', rank), ('target scores', tsc), ('workspace', ws), ('descriptor', desc)] + \
            [('table %d' % s, t) for s, t in enumerate(dt)] + [('valid %d' % s, v) for s, v in enumerate(dv)]:
        if a is not None:
            assert_fence_intact(be, a, name)
    if keep is not None:
        keep['ws'] = be.get(ws)
    return out


def run_per_set(be, pb, k):
    """The oracle: one mpqe_rank_entities_scored call per set over that set's queries, scattered back."""
    from tests.test_rank import csr
    lib = be.lib
    Q, D = pb.q.shape
    out = {'rows': np.full((Q, max(k, 1)), -7, dtype=np.int64), 'scores': np.full((Q, max(k, 1)), np.nan, dtype=np.float32),
           'rank': np.full(Q, -7, dtype=np.int64), 'tscore': np.full(Q, np.nan, dtype=np.float32)}
    sets = np.array([pb.set_of(i) for i in range(Q)])
    for s, table in enumerate(pb.tables):
        idx = np.nonzero(sets == s)[0]
        if idx.size == 0:
            continue
        n, N = int(idx.size), table.shape[0]
        off, rows = csr([pb.excluded(i) for i in idx], n)
        E = int(rows.shape[0])
        dq, dtab, dtg = be.put(pb.q[idx]), be.put(table), be.put(pb.target[idx])
        doff, drows = be.put(off), be.put(rows if E else np.zeros(1, dtype=np.int64))
        topr, tops = be.empty((n, max(k, 1)), np.int64), be.empty((n, max(k, 1)), np.float32)
        rank, tsc = be.empty((n,), np.int64), be.empty((n,), np.float32)
        need = lib.mpqe_rank_workspace_bytes(n, N, D, k)
        ws = be.nbytes(need)
        err = be.zeros((1,), np.int32)
        st = lib.mpqe_rank_entities_scored(be.ptr(dq), n, be.ptr(dtab), N, D, EPS, int(pb.kinds[s]), be.ptr(dtg),
                                           be.ptr(doff), be.ptr(drows), E, k, be.ptr(topr) if k else None,
                                           be.ptr(tops) if k else None, be.ptr(rank), be.ptr(tsc), be.ptr(ws), need,
                                           be.ptr(err), be.stream)
        assert st == 0 and int(be.get(err)[0]) == 0
        if k:
            out['rows'][idx], out['scores'][idx] = be.get(topr), be.get(tops)
        out['rank'][idx], out['tscore'][idx] = be.get(rank), be.get(tsc)
    return out


def same_bits(a, b, k, rows=None, what=''):
    sel = slice(None) if rows is None else rows
    np.testing.assert_array_equal(a['rank'][sel], b['rank'][sel], err_msg=what + ' rank')
    np.testing.assert_array_equal(a['tscore'][sel].view(np.int32), b['tscore'][sel].view(np.int32), err_msg=what + ' target score')
    if k:
        np.testing.assert_array_equal(a['rows'][sel], b['rows'][sel], err_msg=what + ' top-k rows')
        np.testing.assert_array_equal(a['scores'][sel].view(np.int32), b['scores'][sel].view(np.int32),
                                      err_msg=what + ' top-k scores')


@pytest.mark.parametrize('k', [0, 3, MAX_K])
@pytest.mark.parametrize('dim', [20, 128])
def test_equals_the_per_set_calls_to_the_bit(be, dim, k):
    pb = build(10 + dim, dim)
    assert [int((np.array([pb.set_of(i) for i in range(150)]) == s).sum()) for s in range(5)] == list(COUNTS)
    out = run_mixed(be, pb, k)
    assert out['err'] == 0
    same_bits(out, run_per_set(be, pb, k), k)


def test_plain_call_without_bitmaps_and_unaligned_dim(be):
    """No exclusion words, no valid words; dim 7 takes the element-wise loads."""
    for dim in (7, 20):
        pb = build(3, dim, with_bits=False, with_valid=False)
        out = run_mixed(be, pb, 5)
        assert out['err'] == 0
        same_bits(out, run_per_set(be, pb, 5), 5)


def test_a_misaligned_query_matrix_and_partial_blocks(be):
    """Sets of 65 and 130 rows (2 and 3 column tiles, the last one and two rows wide) with 1 and 65 queries: blocks of 1,
    64 and 1 live rows, so the tile core's staging rows past a block stand in for queries that are not there. dim 32 with q
    one float off 16 bytes takes the element-wise loads by the pointer, dim 20 the predicated ones; `valid` and exclusion
    words are present. Every operand sits between fences (run_mixed checks them)."""
    k = 5
    shape = dict(rows=(65, 130), counts=(1, 65))
    pb = build(21, 32, **shape)
    per_set, aligned = run_per_set(be, pb, k), run_mixed(be, pb, k)
    off = run_mixed(be, pb, k, mis_q=1)
    assert aligned['err'] == 0 and off['err'] == 0
    same_bits(aligned, per_set, k, what='dim 32')
    same_bits(off, per_set, k, what='dim 32, q 4 bytes off')
    same_bits(off, aligned, k, what='dim 32, q 4 bytes off against aligned')
    pb = build(22, 20, **shape)
    out = run_mixed(be, pb, k)
    assert out['err'] == 0
    same_bits(out, run_per_set(be, pb, k), k, what='dim 20')


def test_against_float64(be):
    """Cosine sets only (truth() is the cosine): ranks, target scores and top-k inside test_rank.py's tolerance."""
    k = 10
    pb = build(5, 20, kinds=[0] * 5)
    out = run_mixed(be, pb, k)
    assert out['err'] == 0
    sets = np.array([pb.set_of(i) for i in range(pb.q.shape[0])])
    for s, table in enumerate(pb.tables):
        idx = np.nonzero(sets == s)[0]
        if idx.size == 0:
            continue
        s64 = truth(pb.q[idx], table)
        excl = [pb.excluded(i) for i in idx]
        part = {key: out[key][idx] for key in ('rows', 'scores', 'rank', 'tscore')}
        check_topk(part, s64, excl, k)
        check_rank(part, s64, pb.target[idx], excl)


def test_one_set_equals_the_unmixed_call(be):
    k = 7
    pb = build(6, 20, rows=(300,), counts=(97,), kinds=[0])
    out = run_mixed(be, pb, k)
    assert out['err'] == 0
    same_bits(out, run_per_set(be, pb, k), k)


def test_a_shuffle_permutes_the_outputs_and_splits_agree(be):
    k = 3
    pb = build(7, 20)
    Q = pb.q.shape[0]
    whole = run_mixed(be, pb, k)
    perm = np.random.RandomState(1).permutation(Q)
    shuffled = run_mixed(be, pb.take(perm), k)
    same_bits({key: whole[key][perm] for key in ('rows', 'scores', 'rank', 'tscore')}, shuffled, k, what='shuffle')
    lo, hi = run_mixed(be, pb.take(np.arange(77)), k), run_mixed(be, pb.take(np.arange(77, Q)), k)
    joined = {key: np.concatenate([lo[key], hi[key]]) for key in ('rows', 'scores', 'rank', 'tscore')}
    same_bits(whole, joined, k, what='split')


def test_same_call_twice_and_any_workspace_contents(be):
    k = 3
    pb = build(8, 20)
    a = run_mixed(be, pb, k, fill='noise')
    for fill in ('noise', 'ones', 'nan', 'zeros'):
        same_bits(a, run_mixed(be, pb, k, fill=fill), k, what=fill)


def test_everything_but_the_target_excluded(be):
    k = 3
    pb = build(9, 20, with_valid=False)
    Q, W = pb.bits.shape
    dense = np.ones((Q, W * 32), dtype=bool)
    dense[np.arange(Q), pb.target] = False
    pb.bits = np.packbits(dense.reshape(Q, W, 32), axis=2, bitorder='little').view('<u4').reshape(Q, W).view(np.int32)
    out = run_mixed(be, pb, k)
    assert out['err'] == 0
    assert (out['rank'] == 1).all()
    np.testing.assert_array_equal(out['rows'][:, 0], pb.target)
    assert (out['rows'][:, 1:] == -1).all() and np.isneginf(out['scores'][:, 1:]).all()
    np.testing.assert_array_equal(out['scores'][:, 0].view(np.int32), out['tscore'].view(np.int32))
    same_bits(out, run_per_set(be, pb, k), k)


def test_exact_ties_across_a_strip_boundary(be):
    """Copies of one row on both sides of the 700-row set's strip boundaries (a strip is one 64-row tile here) and inside
    the 65-row set's two tiles: the tied rows lead with bit-equal scores, the smaller row first."""
    k = 8
    pb = build(12, 20, kinds=[0, 1, 0, 0, 0], with_bits=False, with_valid=False)
    groups = {4: [5, 63, 64, 130, 699], 3: [0, 63, 64]}
    for s, rows in groups.items():
        for r in rows[1:]:
            pb.tables[s][r] = pb.tables[s][rows[0]]
    sets = np.array([pb.set_of(i) for i in range(pb.q.shape[0])])
    for s, rows in groups.items():
        for i in np.nonzero(sets == s)[0]:
            pb.q[i] = pb.tables[s][rows[0]] * np.float32(2.0) + np.float32(0.01) * pb.q[i]
            pb.target[i] = rows[i % len(rows)]
    out = run_mixed(be, pb, k)
    for s, rows in groups.items():
        for i in np.nonzero(sets == s)[0]:
            n = len(rows)
            assert out['rows'][i, :n].tolist() == sorted(rows), 'query %d: %s' % (i, out['rows'][i])
            assert len(set(out['scores'][i, :n].view(np.int32).tolist())) == 1
            assert out['rank'][i] == 1 + sorted(rows).index(int(pb.target[i]))
    same_bits(out, run_per_set(be, pb, k), k)


def test_bad_groups_and_bad_targets_are_flagged_and_leave_the_rest_intact(be):
    k = 3
    pb = build(14, 20)
    good = run_mixed(be, pb, k)
    assert good['err'] == 0
    Q = pb.q.shape[0]
    sets = np.array([pb.set_of(i) for i in range(Q)])
    bad_g = pb.take(np.arange(Q))
    bad_g.group_of = pb.group_of.copy()
    bad_g.group_of[[4, 77, 149]] = [len(pb.set_of_group), -1, 1 << 40]
    out = run_mixed(be, bad_g, k)
    assert out['err'] & FLAG_BAD_INDEX
    hit = np.array([4, 77, 149])
    keep = np.setdiff1d(np.arange(Q), hit)
    same_bits(out, good, k, rows=keep, what='bad group')
    assert (out['rank'][hit] == -1).all() and np.isnan(out['tscore'][hit]).all()
    assert (out['rows'][hit] == -1).all() and np.isneginf(out['scores'][hit]).all()

    bad_t = pb.take(np.arange(Q))
    bad_t.target = pb.target.copy()
    hit = np.array([int(np.nonzero(sets == 1)[0][0]), int(np.nonzero(sets == 3)[0][2]), int(np.nonzero(sets == 4)[0][1])])
    bad_t.target[hit] = [63, -1, 1 << 33]                  # a row of another set's range, a negative one, a huge one
    out = run_mixed(be, bad_t, k)
    assert out['err'] & FLAG_BAD_INDEX
    keep = np.setdiff1d(np.arange(Q), hit)
    same_bits(out, good, k, rows=keep, what='bad target')
    assert (out['rank'][hit] == -1).all() and np.isnan(out['tscore'][hit]).all()
    np.testing.assert_array_equal(out['rows'], good['rows'])            # the top-k does not depend on the target


def test_a_wide_set_several_tiles_per_strip(be):
    """A 4200-row set has 66 tiles, more than the 64 strips a merging wave can hold: two tiles to a strip (S = 33), while
    the 65-row set of the same call fills two strips and leaves 31 empty. dim 8 keeps the emulator quick."""
    k = 3
    pb = build(15, 8, rows=(65, 4200), counts=(10, 70), kinds=[0, 0])
    out = run_mixed(be, pb, k)
    assert out['err'] == 0
    same_bits(out, run_per_set(be, pb, k), k)


def test_modes_of_the_call(be):
    pb = build(16, 20)
    full = run_mixed(be, pb, 3)
    only_rank = run_mixed(be, pb, 0)
    np.testing.assert_array_equal(only_rank['rank'], full['rank'])
    no_target = pb.take(np.arange(pb.q.shape[0]))
    no_target.target = None
    only_topk = run_mixed(be, no_target, 3)
    np.testing.assert_array_equal(only_topk['rows'], full['rows'])


def test_refusals(be):
    lib = be.lib
    pb = build(17, 20)
    k = 3
    run_mixed(be, pb, k, status=ERR_WORKSPACE, ws_short=1)
    keep = {}
    run_mixed(be, pb, k, fill='nan', status=ERR_WORKSPACE, ws_short=1, keep=keep)
    from tests.fenced import BYTE_FENCE
    assert (keep['ws'] == np.resize(BYTE_FENCE, keep['ws'].shape[0])).all(), 'a refused call wrote to its workspace'
    assert lib.mpqe_rank_mixed_workspace_bytes(150, 5, 700, 893, 20, MAX_K + 1) == 0
    assert lib.mpqe_rank_mixed_workspace_bytes(150, 5, 700, 893, 20, MAX_K) > 0
    assert lib.mpqe_rank_mixed_desc_bytes(0, 4) == 0 and lib.mpqe_rank_mixed_desc_bytes(257, 4) == 0
    assert lib.mpqe_rank_mixed_desc_bytes(256, 1 << 20) > 0 and lib.mpqe_rank_mixed_desc_bytes(1, (1 << 20) + 1) == 0

    # the entries themselves, on small real operands
    num_sets, num_groups = 2, 2
    tables = [be.put(np.ones((5, 20), dtype=np.float32)), be.put(np.ones((9, 20), dtype=np.float32))]
    tabs = (ctypes.c_void_p * 2)(*[be.ptr(t) for t in tables])
    rows = np.array([5, 9], dtype=np.int64)
    kinds = np.array([0, 1], dtype=np.int32)
    sog = np.array([1, 0], dtype=np.int32)
    need_d = lib.mpqe_rank_mixed_desc_bytes(num_sets, num_groups)
    desc = fenced_bytes(be, need_d, 'nan')

    def build_desc(ns=num_sets, ng=num_groups, nbytes=need_d, rows_=rows, kinds_=kinds, sog_=sog):
        return lib.mpqe_rank_mixed_desc_build(tabs, rows_.ctypes.data, kinds_.ctypes.data, None, ns, sog_.ctypes.data, ng,
                                              be.ptr(desc), nbytes, be.stream)
    assert build_desc(ns=0) == ERR_INVALID_ARG
    assert build_desc(ns=257) == ERR_INVALID_ARG
    assert build_desc(ng=0) == ERR_INVALID_ARG
    assert build_desc(rows_=np.array([5, 0], dtype=np.int64)) == ERR_INVALID_ARG
    assert build_desc(kinds_=np.array([0, 2], dtype=np.int32)) == ERR_INVALID_ARG
    assert build_desc(sog_=np.array([1, 2], dtype=np.int32)) == ERR_INVALID_ARG
    assert build_desc(nbytes=need_d - 1) == ERR_WORKSPACE
    held = be.get(desc)
    assert (held == np.resize(BYTE_FENCE, held.shape[0])).all(), 'a refused build wrote to the block'
    assert build_desc() == 0
    assert_fence_intact(be, desc, 'descriptor')

    Q = 4
    q = be.put(np.ones((Q, 20), dtype=np.float32))
    g = be.put(np.zeros(Q, dtype=np.int64))
    tg = be.put(np.zeros(Q, dtype=np.int64))
    topr, tops = be.empty((Q, k), np.int64), be.empty((Q, k), np.float32)
    rank = be.empty((Q,), np.int64)
    need = lib.mpqe_rank_mixed_workspace_bytes(Q, num_sets, 9, 14, 20, k)
    ws = fenced_bytes(be, need, 'noise')
    err = be.zeros((1,), np.int32)

    def call(Q_=Q, k_=k, ns=num_sets, tg_=tg, g_=g, need_=need, nd=need_d):
        return lib.mpqe_rank_entities_mixed(be.ptr(q), Q_, 20, EPS, be.ptr(desc), nd, ns, num_groups, 9, 14, be.ptr(g_),
                                            be.ptr(tg_), None, 0, k_, be.ptr(topr), be.ptr(tops), be.ptr(rank), None,
                                            be.ptr(ws), need_, be.ptr(err), be.stream)
    assert call() == 0
    assert int(be.get(err)[0]) == 0
    assert (be.get(rank) >= 1).all()
    assert call(k_=MAX_K + 1) == ERR_UNSUPPORTED
    assert call(k_=-1) == ERR_INVALID_ARG
    assert call(ns=0) == ERR_INVALID_ARG
    assert call(ns=257) == ERR_INVALID_ARG
    assert call(tg_=None) == ERR_INVALID_ARG                # a rank without targets
    assert call(g_=None) == ERR_INVALID_ARG
    assert call(need_=need - 1) == ERR_WORKSPACE
    assert call(nd=need_d - 1) == ERR_WORKSPACE
    assert call(Q_=-1) == ERR_INVALID_ARG
    assert call(Q_=0) == 0


def test_a_call_that_misnames_the_block_ranks_nothing(be):
    """max_rows / total_rows that are not the block's: flagged, every query as a bad group, no stray access."""
    lib = be.lib
    tables = [be.put(np.ones((5, 20), dtype=np.float32))]
    tabs = (ctypes.c_void_p * 1)(be.ptr(tables[0]))
    rows, kinds, sog = np.array([5], dtype=np.int64), np.array([0], dtype=np.int32), np.array([0], dtype=np.int32)
    need_d = lib.mpqe_rank_mixed_desc_bytes(1, 1)
    desc = fenced_bytes(be, need_d, 'noise')
    assert lib.mpqe_rank_mixed_desc_build(tabs, rows.ctypes.data, kinds.ctypes.data, None, 1, sog.ctypes.data, 1,
                                          be.ptr(desc), need_d, be.stream) == 0
    Q, k = 3, 2
    q, g, tg = be.put(np.ones((Q, 20), dtype=np.float32)), be.put(np.zeros(Q, dtype=np.int64)), be.put(np.zeros(Q, dtype=np.int64))
    topr, tops, rank = be.empty((Q, k), np.int64), be.empty((Q, k), np.float32), be.empty((Q,), np.int64)
    need = lib.mpqe_rank_mixed_workspace_bytes(Q, 1, 4, 4, 20, k)
    ws = fenced_bytes(be, need, 'noise')
    err = be.zeros((1,), np.int32)
    st = lib.mpqe_rank_entities_mixed(be.ptr(q), Q, 20, EPS, be.ptr(desc), need_d, 1, 1, 4, 4, be.ptr(g), be.ptr(tg), None, 0,
                                      k, be.ptr(topr), be.ptr(tops), be.ptr(rank), None, be.ptr(ws), need, be.ptr(err),
                                      be.stream)
    assert st == 0
    assert int(be.get(err)[0]) & FLAG_BAD_INDEX
    assert (be.get(rank) == -1).all() and (be.get(topr) == -1).all()
    assert_fence_intact(be, ws, 'workspace')
