"""csrc/kg_sample.hip through the C ABI (mpqe_kg_sample_queries, mpqe_kg_sample_rows), on the host emulator and (gpu) on
the real library, against tests/kg_sample_oracle.py: the stream and the rules restated with Python ints (bit parity), the
exact single-try distribution of the reference's walk (chi-square; the enumeration is pinned to counts the reference
itself produced, tests/golden/kg_walks_small.npz), and properties that hold whatever the stream is.

Operand hygiene is tests/test_kg_kernels.py's (its helpers are used): outputs sit between guard words that must keep their
bits, outputs and workspace start as garbage, int64 operands start 8 bytes past a 16-byte boundary, 4-byte ones 4 bytes.

The statistical tests use fixed seeds, so they are deterministic; they pass at p >= 1e-6 and print their p-values."""
import ctypes
import json
import os

import numpy as np
import pytest

from mpqe_amd import _capi
from tests import kg_sample_oracle as oracle
from tests import test_kg_kernels as K

be = K.be
BAD_INDEX = _capi.FLAG_BAD_INDEX
OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
P_FLOOR = 1e-6
TYPES = list(range(7))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'kg_walks_small.npz')


class SampleWorld(K.World):
    """K.World plus what the walk takes: the relations' modes and their non-empty source rows (device lists)"""

    def __init__(self, be, mode_rows, relations):
        K.World.__init__(self, be, mode_rows, relations)
        R = len(relations)
        self.src = np.array([r[0] for r in relations], dtype=np.int32)
        self.dst = np.array([r[1] for r in relations], dtype=np.int32)
        starts, counts = [], []
        for src, _, lists in relations:
            rows = np.array(sorted(x for x, l in lists.items() if len(l)), dtype=np.int64)
            d = K._at(be, rows, 8) if rows.size else None
            self.keep.append(d)
            starts.append(be.ptr(d))
            counts.append(rows.size)
        self.starts, self.start_counts = (ctypes.c_void_p * R)(*starts), (ctypes.c_int64 * R)(*counts)

    def d_offsets(self, rel):
        return self.keep[2 * rel]

    def d_rows(self, rel):
        return self.keep[2 * rel + 1]


def _workspace(be, rng, need, misalign):
    """as tests/test_kg_kernels.py's: int64 words here, two int32 more than asked"""
    return K._at(be, K._garbage(rng, need // 4 + 2).view(np.int64), misalign)


def _walk(world, qt, Q, max_tries, seed, rng):
    """one mpqe_kg_sample_queries call -> (records [Q, 10], the error word)"""
    be = world.be
    R, M = len(world.relations), len(world.mode_rows)
    need = be.lib.mpqe_kg_sample_workspace_bytes(R, M)
    assert need >= 256
    ws = _workspace(be, rng, need, 8)
    err = be.zeros((1,), np.int32)
    buf, view, before = K._fenced(be, rng, Q * 10, item=8)
    be.check(be.lib.mpqe_kg_sample_queries(world.offs, world.rows, world.edges, world.src.ctypes.data, world.dst.ctypes.data,
                                           world.starts, world.start_counts, R, world.mode_rows.ctypes.data, M, qt, Q,
                                           max_tries, seed, be.ptr(view), be.ptr(ws), need, be.ptr(err), be.stream),
             'mpqe_kg_sample_queries')
    K._guards_kept(be, buf, before, Q * 10, 'records')
    return be.get(view).reshape(Q, 10).copy(), int(be.get(err)[0])


# ---------------------------------------------------------------------------------------------- worlds
def _world_a_relations(only=None):
    """modes of 5 / 33 / 2 rows. Mode 0: row 0 has flat degree 0, row 1 one entry, row 2 three (2 + 1 over two relations),
    row 3 three in one relation, row 4 two (1 + 1 over two relations). Mode 1: degrees 0 (row 32 and most rows), 1, 2, and
    row 2 whose two entries are the same entry. Mode 2: both rows have degree 1. Relation 5 has no edge."""
    rels = [(0, 1, {1: [4], 2: [7, 9], 3: [1, 2, 3], 4: [5]}),
            (0, 1, {4: [6], 2: [30]}),
            (1, 0, {4: [1], 7: [2, 0], 9: [3], 1: [0], 2: [4, 4], 5: [3, 1]}),
            (1, 2, {5: [0], 6: [1], 30: [1, 0], 3: [0]}),
            (2, 1, {0: [32], 1: [32]}),
            (2, 0, {}),
            (1, 1, {7: [30]})]
    if only is not None:
        rels = [(s, d, lists if i in only else {}) for i, (s, d, lists) in enumerate(rels)]
    return rels


ROWS_A = [5, 33, 2]


@pytest.fixture(scope='module')
def golden():
    z = np.load(GOLDEN)
    info = json.loads(bytes(z['meta']).decode())
    modes = info['modes']
    row_of, mode_of = {}, {}
    for m in modes:
        for r, i in enumerate(info['ids'][m]):
            row_of[i], mode_of[i] = r, modes.index(m)
    typed = [tuple(r) for r in info['typed_relations']]
    relations = [(modes.index(r[0]), modes.index(r[2]), {}) for r in typed]
    for r, s, d in zip(z['adj_rel'], z['adj_src'], z['adj_dst']):
        relations[int(r)][2].setdefault(row_of[int(s)], []).append(row_of[int(d)])
    recorded = {}
    for t in range(1, 7):
        counts = {}
        for rec, c in zip(z['out_%d' % t], z['cnt_%d' % t]):
            key = None if rec[0] < 0 else tuple(int(v) if i % 3 == 1 else row_of[int(v)] for i, v in enumerate(rec) if v >= 0)
            counts[key] = int(c)
        recorded[t] = counts
    return {'mode_rows': [len(info['ids'][m]) for m in modes], 'relations': relations, 'recorded': recorded,
            'tries': info['tries'], 'dist': {t: oracle.single_try_distribution(relations, t) for t in TYPES}}


# ---------------------------------------------------------------------------------------------- 1. bit parity
@pytest.mark.parametrize('qt', TYPES)
def test_walk_equals_the_restated_stream(be, qt):
    world = SampleWorld(be, ROWS_A, _world_a_relations())
    rng = np.random.RandomState(qt)
    some = 0
    for Q in (1, 255, 257):
        for max_tries in (1, 8):
            for seed in (5, 2 ** 63 + 12345):
                got, err = _walk(world, qt, Q, max_tries, seed, rng)
                want = oracle.walk(world.relations, qt, Q, max_tries, seed)
                np.testing.assert_array_equal(got, want, err_msg='Q %d, max_tries %d, seed %d' % (Q, max_tries, seed))
                assert err == 0
                some += int(got[:, 0].sum())
    assert some > 0


def test_walk_from_a_mode_of_degree_one_finds_no_3_inter(be):
    """only relation 4 (mode 2 -> mode 1, both rows of degree 1) has edges: every start has one entry, 3-inter needs three"""
    world = SampleWorld(be, ROWS_A, _world_a_relations(only=(4,)))
    got, err = _walk(world, 4, 257, 8, 77, np.random.RandomState(1))
    assert err == 0
    np.testing.assert_array_equal(got[:, 0], 0)
    np.testing.assert_array_equal(got[:, 1:], -1)
    np.testing.assert_array_equal(got, oracle.walk(world.relations, 4, 257, 8, 77))
    one, err = _walk(world, 0, 257, 1, 77, np.random.RandomState(2))          # a 1-chain is found at once
    assert err == 0 and (one[:, 0] == 1).all() and (one[:, 2] == 4).all() and (one[:, 3] == 32).all()


# ---------------------------------------------------------------------------------------------- 2. structure
def _check_shape(relations, mode_rows, qt, rec):
    """a status-1 record is a subgraph of the world of its type's shape -> its edges"""
    n_edges = {0: 1, 1: 2, 2: 3, 3: 2, 4: 3, 5: 3, 6: 3}[qt]
    vals = rec[1:1 + 3 * n_edges].tolist()
    assert all(v >= 0 for v in vals) and (rec[1 + 3 * n_edges:] == -1).all()
    edges = [tuple(vals[3 * i:3 * i + 3]) for i in range(n_edges)]
    for x, r, y in edges:
        src, dst, lists = relations[r]
        assert 0 <= x < mode_rows[src] and 0 <= y < mode_rows[dst] and y in lists.get(x, ())
    frm = {0: [], 1: [0], 2: [0, 1], 3: [None], 4: [None, None], 5: [None, 1], 6: [0, 0]}[qt]     # edge i + 1 starts at ...
    for i, f in enumerate(frm):
        x, r, _ = edges[i + 1]
        if f is None:
            assert x == edges[0][0] and relations[r][0] == relations[edges[0][1]][0]
        else:
            assert x == edges[f][2] and relations[r][0] == relations[edges[f][1]][1]
    for fan in {3: [(0, 1)], 4: [(0, 1, 2)], 5: [(0, 1)], 6: [(1, 2)]}.get(qt, []):     # the edges drawn out of one node
        assert len(set(edges[i][0] for i in fan)) == 1
        assert len(set(edges[i][1:] for i in fan)) == len(fan)          # ... differ in (relation, neighbour)
    return edges


def _programme_of(qt, edges):
    """(branches [(anchor's relation index side ...)], tail, anchors) with relation i's inverse at index i ^ 1"""
    rev = lambda e: e[1] ^ 1                                          # noqa: E731
    if qt in (0, 1, 2):
        return [[rev(e) for e in reversed(edges)]], [], [edges[-1][2]]
    if qt in (3, 4):
        return [[rev(e)] for e in edges], [], [e[2] for e in edges]
    if qt == 5:
        return [[rev(edges[0])], [rev(edges[2]), rev(edges[1])]], [], [edges[0][2], edges[2][2]]
    return [[rev(edges[1])], [rev(edges[2])]], [rev(edges[0])], [edges[1][2], edges[2][2]]


@pytest.mark.parametrize('qt', TYPES)
def test_records_are_subgraphs_whose_target_answers_them(be, golden, qt):
    """Independent of the stream: every status-1 record is a subgraph of the world of its type's shape, its modes chain,
    edges out of one node differ, and mpqe_kg_answers on the same world, for the formula / anchors rebuilt from the record,
    holds the target's bit. (The golden's graph: closed under inverse, relation i's inverse is relation i ^ 1.)"""
    world = SampleWorld(be, golden['mode_rows'], golden['relations'])
    rng = np.random.RandomState(30 + qt)
    got, err = _walk(world, qt, 257, 8, 1000 + qt, rng)
    assert err == 0 and got[:, 0].sum() > 200
    by_formula = {}
    for rec in got:
        if rec[0] == 0:
            assert (rec[1:] == -1).all()
            continue
        edges = _check_shape(world.relations, world.mode_rows, qt, rec)
        hops, tail, anchors = _programme_of(qt, edges)
        by_formula.setdefault((tuple(map(tuple, hops)), tuple(tail)), []).append((anchors, edges[0][0]))
    for (hops, tail), members in sorted(by_formula.items())[:12]:
        branches = [(world.relations[h[0]][0], list(h)) for h in hops]
        prog, target_mode = world.programme(branches, list(tail))
        anchors = np.array([m[0] for m in members], dtype=np.int64).T
        n_out = int(world.mode_rows[target_mode])
        answers, _, _, err = K._call(world, prog, anchors, n_out, rng, 0)
        assert err == 0
        for q, (_, target) in enumerate(members):
            assert (answers[q, target >> 5] >> (target & 31)) & 1, (qt, hops, tail, members[q])


# ---------------------------------------------------------------------------------------------- 3. bounded redraw
def test_a_repeated_entry_ends_the_redraws(be):
    """The only row that can start has a flat list of ONE (relation, neighbour) entry, twice: the second edge of a 2-inter
    can never differ. Every slot gives up (KGS_MAX_REDRAWS) and reports status 0; the call returns. Run once, no time limit
    involved. Mutant: the redraw bound removed -- this test does not return on the emulator (never run that on a GPU)."""
    world = SampleWorld(be, [3, 4], [(0, 1, {1: [2, 2]}), (1, 0, {})])
    got, err = _walk(world, 3, 257, 8, 9, np.random.RandomState(3))
    assert err == 0
    np.testing.assert_array_equal(got[:, 0], 0)
    np.testing.assert_array_equal(got[:, 1:], -1)
    one, err = _walk(world, 0, 5, 1, 9, np.random.RandomState(4))
    assert err == 0 and one[:, 1:4].tolist() == [[1, 0, 2]] * 5


# ---------------------------------------------------------------------------------------------- 4. distribution
@pytest.mark.parametrize('qt', TYPES)
def test_single_try_distribution(be, golden, qt):
    """max_tries = 1, 20 000 slots: the outcome counts (None included) against the EXACT distribution of one try of the
    reference's walk, enumerated by the oracle; outcomes of expected count < 5 pooled. The reference's own recorded counts
    go through the same statistic against the same enumeration, which pins the enumeration to the reference and not to the
    code under test (the reference has no 1-chain walk: kernel only).
    Mutant this catches: drawing a relation out of the node uniformly and then a neighbour in it, instead of uniformly over
    the flat list -- rows whose degree differs between two relations then favour the sparser relation's entries."""
    world = SampleWorld(be, golden['mode_rows'], golden['relations'])
    dist = golden['dist'][qt]
    if qt:
        stat, dof, p = oracle.chi_square(golden['recorded'][qt], dist, golden['tries'])
        print('reference %s: chi2 %.1f, dof %d, p %.3g' % (oracle.QUERY_TYPES[qt], stat, dof, p))
        assert p >= P_FLOOR
    Q = 20000
    got, err = _walk(world, qt, Q, 1, 4242 + qt, np.random.RandomState(40 + qt))
    assert err == 0
    stat, dof, p = oracle.chi_square(oracle.counts_of(got), dist, Q)
    print('kernel %s (%s): chi2 %.1f, dof %d, p %.3g' % (oracle.QUERY_TYPES[qt], be.name, stat, dof, p))
    assert p >= P_FLOOR


def test_the_statistic_rejects_uniform_over_relations(golden):
    """the mutant of test_single_try_distribution, simulated on the host: its counts fail the same statistic"""
    rng = np.random.RandomState(0)
    relations = golden['relations']
    counts = {}
    for _ in range(20000):
        active = [i for i, r in enumerate(relations) if r[2]]
        r0 = active[rng.randint(len(active))]
        starts = sorted(relations[r0][2])
        x = starts[rng.randint(len(starts))]
        out = [i for i, r in enumerate(relations) if r[0] == relations[r0][0] and r[2].get(x)]
        r = out[rng.randint(len(out))]
        y = relations[r][2][x][rng.randint(len(relations[r][2][x]))]
        counts[(x, r, y)] = counts.get((x, r, y), 0) + 1
    assert oracle.chi_square(counts, golden['dist'][0], 20000)[2] < P_FLOOR


# ---------------------------------------------------------------------------------------------- 5. corrupt CSR
@pytest.mark.parametrize('qt', TYPES)
def test_corrupt_csr_is_flagged_and_not_followed(be, qt):
    """relation 0's last offset points beyond its edges, and relation 2 lists a row >= n_dst: MPQE_FLAG_BAD_INDEX, and no
    record names a row outside its mode; the tries that do not meet them still give queries"""
    world = SampleWorld(be, ROWS_A, _world_a_relations())
    off0 = world.d_offsets(0)
    off0[5] = int(world.edges[0]) + 5              # row 4's list: [lo, edges + 5)
    rows2 = world.d_rows(2)
    rows2[1] = 5                                   # relation 2, row 1: neighbour 5 of a mode of 5 rows
    flagged = 0
    for seed in (1, 2):
        got, err = _walk(world, qt, 257, 8, seed, np.random.RandomState(seed))
        flagged |= err
        assert err in (0, BAD_INDEX)
        for rec in got[got[:, 0] == 1]:
            edges = _check_shape(world.relations, world.mode_rows, qt, rec)
            assert all((x, r) != (4, 0) for x, r, _ in edges)
    assert flagged == BAD_INDEX


# ---------------------------------------------------------------------------------------------- mpqe_kg_sample_rows
def _sample_rows(be, rng, bits, n, valid, select, lengths, k, seed, slack=1):
    """-> (offsets, the rows [total], error word); as K._rows_call"""
    Q = bits.shape[0]
    off = np.zeros(Q + 1, dtype=np.int64)
    off[1:] = np.cumsum(lengths)
    total = int(off[-1])
    d_bits = K._at(be, bits.view(np.int32), 4)
    d_valid = None if valid is None else K._at(be, valid.view(np.int32), 4)
    d_off = K._at(be, off, 8)
    buf, view, before = K._fenced(be, rng, total + slack + 1, item=8)
    err = be.zeros((1,), np.int32)
    be.check(be.lib.mpqe_kg_sample_rows(be.ptr(d_bits), Q, n, be.ptr(d_valid), select, be.ptr(d_off), be.ptr(view),
                                        total + slack, k, seed, be.ptr(err), be.stream), 'mpqe_kg_sample_rows')
    K._guards_kept(be, buf, before, total + slack + 1, 'rows_out')
    out = be.get(view)
    np.testing.assert_array_equal(out[total:], before[K.GUARD + total:K.GUARD + total + slack + 1], err_msg='slots behind the lists')
    return off, out[:total].copy(), int(be.get(err)[0])


def _pack(member, stray=True):
    Q, n = member.shape
    W = K._words(n)
    pad = np.full((Q, W * 32 - n), stray, dtype=bool)                 # stray bits behind row n - 1
    return np.packbits(np.concatenate([member, pad], axis=1), axis=1, bitorder='little').view(np.uint32).reshape(Q, W)


def _sets(rng, n):
    """empty, full, row 0 alone, row n - 1 alone, sparse, dense, and every row but the last"""
    member = np.zeros((7, n), dtype=bool)
    member[1] = True
    member[2, 0] = True
    member[3, n - 1] = True
    member[4] = rng.rand(n) < 0.3
    member[5] = rng.rand(n) < 0.9
    member[6, :n - 1] = True
    return member


@pytest.mark.parametrize('k', [1, 3, 100, _capi.KG_SAMPLE_MAX_K])
@pytest.mark.parametrize('n', [1, 31, 32, 33, 70, 2500])
def test_sample_rows(be, n, k):
    """Both selects, `valid` with holes (and none). c <= k: the list of mpqe_kg_rows to the bit. c > k: exactly k rows,
    distinct, members of the selected set (never a hole, never a row >= n), equal to the oracle's restatement, and not
    changed by what the other queries of the batch hold. n = 2 500 is 79 words: two chunks of 64.
    Mutants: the complement forgetting `valid` (holes come out: membership and the oracle fail), the rank select off by
    one at a word boundary (n = 70 and 2 500: a wrong or non-member row), a k-subset that repeats a member (distinct)."""
    rng = np.random.RandomState(1000 * k + n)
    member = _sets(rng, n)
    Q = member.shape[0]
    is_valid = rng.rand(n) < 0.8
    is_valid[n - 1] = True
    is_valid[0] = n < 3 or is_valid[0]
    bits = _pack(member)
    valid = _pack(is_valid[None, :])[0]
    swapped_member = ~member
    swapped_member[4] = member[4]
    swapped = _pack(swapped_member)
    seed = 7 + n

    def chosen_of(member, select, vmap):
        if select == _capi.KG_ROWS_SET:
            return member
        return ~member & (is_valid[None, :] if vmap is not None else True)
    for select, vmap in ((_capi.KG_ROWS_SET, valid), (_capi.KG_ROWS_SET, None), (_capi.KG_ROWS_COMPLEMENT, valid),
                         (_capi.KG_ROWS_COMPLEMENT, None)):
        chosen = chosen_of(member, select, vmap)
        c = chosen.sum(axis=1)
        lengths = np.minimum(c, k)
        off, rows, err = _sample_rows(be, rng, bits, n, vmap, select, lengths, k, seed)
        assert err == 0
        full_off, full_rows, full_err = K._rows_call(be, rng, bits, n, vmap, select, c)
        assert full_err == 0
        for q in range(Q):
            mine = rows[off[q]:off[q + 1]]
            members = np.nonzero(chosen[q])[0]
            what = 'select %d, query %d' % (select, q)
            if c[q] <= k:
                np.testing.assert_array_equal(mine, full_rows[full_off[q]:full_off[q + 1]], err_msg=what)
                np.testing.assert_array_equal(mine, members, err_msg=what)
            else:
                assert mine.shape[0] == k == len(set(mine.tolist())), what
                assert set(mine.tolist()) <= set(members.tolist()), what
                np.testing.assert_array_equal(mine, oracle.sample_rows(members.tolist(), k, seed, q), err_msg=what)
        # the same set at the same position of a batch whose other queries hold other sets
        c2 = chosen_of(swapped_member, select, vmap).sum(axis=1)
        off2, rows2, err = _sample_rows(be, rng, swapped, n, vmap, select, np.minimum(c2, k), k, seed)
        assert err == 0
        np.testing.assert_array_equal(rows2[off2[4]:off2[5]], rows[off[4]:off[5]])


def test_sample_rows_of_answers_from_both_homes(be):
    """bits as mpqe_kg_answers writes them, working bitmaps in LDS and in the workspace: the same sampled rows"""
    world = K._seven_world(be)
    branches, tail = K.SEVEN['3-chain_inter']
    prog, target = world.programme(branches, tail)
    n = int(world.mode_rows[target])
    rng = np.random.RandomState(8)
    anchors = np.stack([rng.randint(0, world.mode_rows[m], size=9) for m, _ in branches])
    out = []
    for flags in (0, _capi.KG_GLOBAL_BITS):
        answers, hard, counts, err = K._call(world, prog, anchors, n, rng, flags)
        assert err == 0
        neg = _sample_rows(be, rng, answers, n, None, _capi.KG_ROWS_COMPLEMENT, np.minimum(n - counts[0], 5), 5, 3)
        hrd = _sample_rows(be, rng, hard, n, None, _capi.KG_ROWS_SET, np.minimum(counts[1], 2), 2, 3)
        assert neg[2] == 0 and hrd[2] == 0
        out.append((neg[1], hrd[1], answers, hard))
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])
    assert out[0][0].shape[0] == 45 and out[0][1].shape[0] > 0
    for q in range(9):
        members = [r for r in range(n) if not (out[0][2][q, r >> 5] >> (r & 31)) & 1]
        np.testing.assert_array_equal(out[0][0][5 * q:5 * q + 5], oracle.sample_rows(members, 5, 3, q))


def test_sampled_subsets_are_uniform(be):
    """One set of c = 40 members of a mode of 70 rows, k = 7, 20 000 query positions. Inclusion: the count of every member
    against N k / c. The 7 rows of a query are distinct, so the counts are not multinomial: their covariance is
    p (1 - p) c / (c - 1) (I - J / c) with p = k / c, and Pearson's sum times (c - 1) / (c - k) is chi-square with c - 1
    degrees of freedom. Pairs: members of adjacent rank come out together with probability k (k - 1) / (c (c - 1)) (a
    bijection that is only a rotation would give (k - 1) / c); a binomial count, tested at the normal quantile of
    p = 1e-6 (4.89 sigma), as is a pair of distant rank."""
    rng = np.random.RandomState(12)
    n, c, k, N = 70, 40, 7, 20000
    members = np.sort(rng.choice(n, size=c, replace=False))
    one = np.zeros((1, n), dtype=bool)
    one[0, members] = True
    bits = np.repeat(_pack(one), N, axis=0)
    off, rows, err = _sample_rows(be, rng, bits, n, None, _capi.KG_ROWS_SET, np.full(N, k), k, 99)
    assert err == 0
    rows = rows.reshape(N, k)
    assert all(len(set(r)) == k for r in rows[:500].tolist()) and np.isin(rows, members).all()
    counts = np.array([(rows == m).sum() for m in members])
    assert counts.sum() == N * k
    e = N * k / c
    stat = float(((counts - e) ** 2 / e).sum()) * (c - 1) / (c - k)
    p = oracle._gammaincc((c - 1) / 2.0, stat / 2.0)
    print('inclusion (%s): chi2 %.1f, dof %d, p %.3g' % (be.name, stat, c - 1, p))
    assert p >= P_FLOOR
    pair_p = k * (k - 1) / (c * (c - 1))
    for a, b in ((members[3], members[4]), (members[0], members[25])):
        both = int(((rows == a).any(axis=1) & (rows == b).any(axis=1)).sum())
        z = (both - N * pair_p) / np.sqrt(N * pair_p * (1 - pair_p))
        print('pair (%d, %d): %d together, expected %.1f, z %.2f' % (a, b, both, N * pair_p, z))
        assert abs(z) <= 4.89


def test_sample_rows_with_wrong_offsets(be):
    """segments one slot shorter and one longer than m = min(k, c): MPQE_FLAG_BAD_INDEX, nothing lands outside a query's
    own segment (_sample_rows checks the guards and the slack), the other queries are exact"""
    rng = np.random.RandomState(2)
    n, k = 70, 4
    member = rng.rand(4, n) < 0.5
    member[3] = False
    member[3, :3] = True                                               # c = 3 < k
    bits = _pack(member, stray=False)
    true = np.minimum(member.sum(axis=1), k)
    for delta in ([0, -1, 1, 0], [0, 0, 0, 1], [0, 0, 0, -1]):
        lengths = true + np.array(delta)
        off, rows, err = _sample_rows(be, rng, bits, n, None, _capi.KG_ROWS_SET, lengths, k, 5)
        assert err == BAD_INDEX
        for q in range(4):
            want = oracle.sample_rows(np.nonzero(member[q])[0].tolist(), k, 5, q)
            m = min(len(want), int(lengths[q]))
            np.testing.assert_array_equal(rows[off[q]:off[q] + m], want[:m])
    off, rows, err = _sample_rows(be, rng, bits, n, None, _capi.KG_ROWS_SET, true, k, 5)
    assert err == 0


# ---------------------------------------------------------------------------------------------- argument checks, no launch
def _libs():
    from mpqe_amd import _lib
    from tests.kernel_backend import EmuBackend
    return {'emu': lambda: EmuBackend().lib, 'product': _lib.load}


@pytest.mark.parametrize('which', ['emu', 'product'])
def test_entry_points_refuse_before_any_launch(which):
    """Device pointers are made-up addresses: a call that launched anything with them would fault."""
    lib = _libs()[which]()
    fake = 0x10000

    def rows_call(bits=fake, Q=5, n=40, valid=fake, select=0, offsets=fake, out=fake, cap=10, k=3):
        return lib.mpqe_kg_sample_rows(bits, Q, n, valid, select, offsets, out, cap, k, 1, None, None)
    assert rows_call(select=_capi.KG_ROWS_WITH_HOLES) == INVALID and rows_call(select=-1) == INVALID
    assert rows_call(k=0) == INVALID and rows_call(k=-3) == INVALID
    assert rows_call(k=_capi.KG_SAMPLE_MAX_K + 1) == UNSUPPORTED
    assert rows_call(n=_capi.KG_SAMPLE_MAX_ROWS + 1) == UNSUPPORTED
    assert rows_call(bits=None) == INVALID and rows_call(offsets=None) == INVALID and rows_call(out=None) == INVALID
    assert rows_call(Q=-1) == INVALID and rows_call(n=0) == INVALID and rows_call(cap=-1) == INVALID
    assert rows_call(Q=0) == OK and rows_call(Q=0, k=_capi.KG_SAMPLE_MAX_K, n=_capi.KG_SAMPLE_MAX_ROWS) == OK
    assert _capi.KG_SAMPLE_MAX_K >= 1024 and _capi.KG_SAMPLE_MAX_ROWS >= 4 << 20

    R = 3
    ptrs = (ctypes.c_void_p * R)(fake, fake, fake)
    edges = (ctypes.c_int64 * R)(7, 7, 0)
    starts = (ctypes.c_int64 * R)(2, 3, 0)
    src, dst = np.array([0, 1, 0], dtype=np.int32), np.array([1, 0, 0], dtype=np.int32)
    mode_rows = np.array([40, 100000], dtype=np.int64)

    def walk(offs=ptrs, rows=ptrs, edges=edges, src=src, dst=dst, start=ptrs, starts=starts, R=R, mode_rows=mode_rows, M=2,
             qt=3, Q=5, tries=8, out=fake, ws=fake, wb=1 << 20):
        return lib.mpqe_kg_sample_queries(offs, rows, edges, None if src is None else src.ctypes.data,
                                          None if dst is None else dst.ctypes.data, start, starts, R,
                                          None if mode_rows is None else mode_rows.ctypes.data, M, qt, Q, tries, 1, out, ws,
                                          wb, None, None)
    need = lib.mpqe_kg_sample_workspace_bytes(R, 2)
    assert need >= 256 and lib.mpqe_kg_sample_workspace_bytes(0, 2) == 0 and lib.mpqe_kg_sample_workspace_bytes(3, 17) == 0
    assert lib.mpqe_kg_sample_workspace_bytes(100, 6) <= 16384
    assert walk(offs=None) == INVALID and walk(rows=None) == INVALID and walk(edges=None) == INVALID
    assert walk(src=None) == INVALID and walk(dst=None) == INVALID and walk(start=None) == INVALID
    assert walk(starts=None) == INVALID and walk(mode_rows=None) == INVALID
    assert walk(R=0) == INVALID and walk(M=0) == INVALID and walk(M=17) == INVALID and walk(M=1) == INVALID
    assert walk(qt=-1) == INVALID and walk(qt=7) == INVALID and walk(Q=-1) == INVALID
    assert walk(tries=0) == INVALID and walk(tries=1025) == INVALID
    assert walk(src=np.array([0, 2, 0], dtype=np.int32)) == INVALID
    assert walk(edges=(ctypes.c_int64 * R)(7, -1, 0)) == INVALID
    assert walk(starts=(ctypes.c_int64 * R)(2, 8, 0)) == INVALID                  # more start rows than edges
    assert walk(starts=(ctypes.c_int64 * R)(41, 3, 0)) == INVALID                 # ... than rows of the mode
    assert walk(offs=(ctypes.c_void_p * R)(fake, None, fake)) == INVALID
    assert walk(start=(ctypes.c_void_p * R)(fake, None, fake)) == INVALID
    assert walk(out=None) == INVALID and walk(ws=None) == INVALID and walk(ws=fake + 4) == INVALID
    assert walk(wb=need - 1) == WORKSPACE
    assert walk(Q=0) == OK and walk(Q=0, out=None, ws=None) == OK
