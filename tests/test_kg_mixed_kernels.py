"""Queries of DIFFERENT formulas in one launch, through the C ABI (mpqe_kg_table_build, mpqe_kg_answers_mixed,
mpqe_kg_sample_rows_mixed; csrc/kg.hip, csrc/kg_sample.hip), on the host emulator and (gpu) on the real library.

The oracle of the answers is tests/kg_oracle.py's Python sets, walked in the hop order kg.query_hops gives for the Formula a
record spells; the same queries also go, one by one, through mpqe_kg_answers with the programme of that formula. The oracle
of the draws is tests/kg_sample_oracle.py's restatement, and mpqe_kg_sample_rows per mode. Every comparison is exact, on
whole words. Operand hygiene is tests/test_kg_kernels.py's (its helpers are used): outputs between guard words, outputs and
workspace start as random bits, 4-byte operands 4 bytes past a 16-byte boundary, int64 ones 8 bytes past one."""
import ctypes

import numpy as np
import pytest

from mpqe_amd import _capi
from mpqe_amd.graph import Formula, reverse_relation
from mpqe_amd.kg import query_hops
from tests import kg_oracle
from tests import kg_sample_oracle as oracle
from tests import test_kg_kernels as K
from tests import test_kg_sample_kernels as T

be = K.be
BAD_INDEX = _capi.FLAG_BAD_INDEX
OK, INVALID, WORKSPACE = 0, -1, -3
TYPES = list(_capi.QUERY_TYPE_IDS)
# per query type: the edge whose neighbour an edge starts from (-1: the target), in the record's edge order
PARENT = {'1-chain': [-1], '2-chain': [-1, 0], '3-chain': [-1, 0, 1], '2-inter': [-1, -1], '3-inter': [-1, -1, -1],
          '3-inter_chain': [-1, -1, 1], '3-chain_inter': [-1, 0, 0]}
ANCHOR_EDGES = {'1-chain': [0], '2-chain': [1], '3-chain': [2], '2-inter': [0, 1], '3-inter': [0, 1, 2],
                '3-inter_chain': [0, 2], '3-chain_inter': [1, 2]}
ROWS = [1, 33, 65]
ROW_ID_STEP = 7


def _poke(arr, i, v):
    arr[i] = v


class MixedWorld(K.World):
    """K.World over named relations ('m<src>', name, 'm<dst>') plus the device table. pairs: (src, dst, name, lists) -- the
    relation and, unless the modes are equal (then the lists are made symmetric and the relation is its own reverse), its
    inverse under the same name; lone: relations WITHOUT a reverse in the index."""

    def __init__(self, be, mode_rows, pairs, lone=()):
        names, rels = [], []
        for s, d, name, lists in pairs:
            if s == d:
                sym = {}
                for x, l in lists.items():
                    for y in l:
                        sym.setdefault(x, []).append(y)
                        sym.setdefault(y, []).append(x)
                names.append(('m%d' % s, name, 'm%d' % d))
                rels.append((s, d, sym))
                continue
            inv = {}
            for x in sorted(lists):
                for y in lists[x]:
                    inv.setdefault(y, []).append(x)
            names += [('m%d' % s, name, 'm%d' % d), ('m%d' % d, name, 'm%d' % s)]
            rels += [(s, d, lists), (d, s, inv)]
        for s, d, name, lists in lone:
            names.append(('m%d' % s, name, 'm%d' % d))
            rels.append((s, d, lists))
        K.World.__init__(self, be, mode_rows, rels)
        self.names = names
        self.index = {n: i for i, n in enumerate(names)}
        self.lists = {n: rels[i][2] for i, n in enumerate(names)}
        self.reverse = np.array([self.index.get(reverse_relation(n), -1) for n in names], dtype=np.int32)
        self.src = np.array([r[0] for r in rels], dtype=np.int32)
        self.dst = np.array([r[1] for r in rels], dtype=np.int32)
        rng = np.random.RandomState(len(names))
        M = len(mode_rows)
        self.is_valid = [rng.rand(n) < 0.8 for n in mode_rows]
        for v in self.is_valid:
            v[-1] = True
        self.row_ids = [1000 * m + ROW_ID_STEP * np.arange(n, dtype=np.int64) for m, n in enumerate(mode_rows)]
        self.d_valid = [K._at(be, T._pack(v[None, :])[0].view(np.int32), 4) for v in self.is_valid]
        self.d_row_ids = [K._at(be, r, 8) for r in self.row_ids]
        self.valid_ptrs = (ctypes.c_void_p * M)(*[be.ptr(v) for v in self.d_valid])
        self.row_id_ptrs = (ctypes.c_void_p * M)(*[be.ptr(r) for r in self.d_row_ids])
        self.build_table()

    def build_table(self, rng=None):
        be, R, M = self.be, len(self.relations), len(self.mode_rows)
        need = be.lib.mpqe_kg_table_bytes(R, M)
        assert need >= 256 and need % 8 == 0
        self.table_buf, self.table, self.table_before = K._fenced(be, rng or np.random.RandomState(1), need // 8, item=8)
        self.table_need = need
        be.check(be.lib.mpqe_kg_table_build(self.offs, self.rows, self.edges, self.src.ctypes.data, self.dst.ctypes.data,
                                            self.reverse.ctypes.data, R, self.mode_rows.ctypes.data, self.valid_ptrs,
                                            self.row_id_ptrs, M, be.ptr(self.table), need, be.stream), 'mpqe_kg_table_build')
        K._guards_kept(be, self.table_buf, self.table_before, need // 8, 'the table')

    # ---- records and their oracle
    def formula(self, qt, rel_ids):
        rels = [self.names[int(r)] for r in rel_ids]
        return Formula(qt, tuple(rels) if qt.endswith('-chain') or qt.endswith('-inter') else (rels[0], (rels[1], rels[2])))

    def random_records(self, qt, Q, rng):
        """Q records of pairwise different relation tuples: a typed walk from a random target row; a neighbour is taken
        from the row's list where it has one (so that sets are not all empty), else it is any row of the mode"""
        out, seen = [], set()
        parent = PARENT[qt]
        for _ in range(10000):
            if len(out) == Q:
                break
            rec = np.full(_capi.KG_QUERY_INTS, -1, dtype=np.int64)
            mode0 = int(rng.randint(len(self.mode_rows)))
            x0 = int(rng.randint(self.mode_rows[mode0]))
            ys, ok = [], True
            for e, p in enumerate(parent):
                mode, x = (mode0, x0) if p < 0 else (int(self.dst[rec[2 + 3 * p]]), ys[p])
                cand = [i for i in range(len(self.names)) if self.src[i] == mode and self.reverse[i] >= 0]
                if not cand:
                    ok = False
                    break
                r = int(cand[rng.randint(len(cand))])
                l = self.relations[r][2].get(x, ())
                y = int(l[rng.randint(len(l))]) if len(l) else int(rng.randint(self.mode_rows[self.dst[r]]))
                rec[1 + 3 * e:4 + 3 * e] = (x, r, y)
                ys.append(y)
            key = tuple(rec[2:2 + 3 * len(parent):3])
            if not ok or key in seen:
                continue
            seen.add(key)
            rec[0] = 1
            out.append(rec)
        assert len(out) == Q, 'the world has fewer than %d relation tuples of %s' % (Q, qt)
        return np.stack(out)

    def sets_of(self, qt, rec):
        """(answers, hard, target mode) of one good record by the Python-set oracle, hops in kg.query_hops' order"""
        n_e = len(PARENT[qt])
        formula = self.formula(qt, rec[2:2 + 3 * n_e:3])
        anchors = [int(rec[3 + 3 * e]) for e in ANCHOR_EDGES[qt]]
        branches, tail = query_hops(formula)
        both, some = kg_oracle.programme_sets([[self.lists[r] for r in hops] for _, hops in branches],
                                              [self.lists[r] for r in tail], [anchors[slot] for slot, _ in branches])
        return both, some - both, int(formula.target_mode[1:])

    def per_formula(self, qt, rec, rng):
        """the same query through mpqe_kg_answers with the programme of its formula -> (answers [W], hard [W], counts)"""
        n_e = len(PARENT[qt])
        formula = self.formula(qt, rec[2:2 + 3 * n_e:3])
        anchors = [int(rec[3 + 3 * e]) for e in ANCHOR_EDGES[qt]]
        branches, tail = query_hops(formula)
        prog, target = self.programme([(int(hops[0][0][1:]), [self.index[r] for r in hops]) for _, hops in branches],
                                      [self.index[r] for r in tail])
        a, h, c, err = K._call(self, prog, np.array([[anchors[slot]] for slot, _ in branches]), int(self.mode_rows[target]),
                               rng, 0)
        assert err == 0
        return a[0], h[0], c[:, 0]


def _pairs(rng, hub=False):
    def lists(s, d, deg=4):
        return K._random_lists(rng, ROWS[s], ROWS[d], deg)
    p = [(0, 1, 'a', lists(0, 1, 9)), (1, 2, 'b', lists(1, 2)), (0, 2, 'c', lists(0, 2, 12)), (2, 1, 'd', lists(2, 1)),
         (1, 1, 'e', lists(1, 1, 3)), (2, 2, 'f', lists(2, 2, 3)), (1, 2, 'g', lists(1, 2, 2))]
    if hub:                                 # a row of degree 1 000 (repeats: 65 rows to land on), rows without a list
        p[1][3][5] = rng.randint(0, 65, size=1000).tolist()
        p[1][3].pop(6, None)
        p[3][3][64] = [5] * 3 + rng.randint(0, 33, size=70).tolist()
        p[4][3][5] = [8, 6]
    return p


def _world(be, hub=False, lone=()):
    return MixedWorld(be, ROWS, _pairs(np.random.RandomState(23), hub), lone)


def _mixed_call(world, qt, records, rng, flags=0, extra_words=0, probe=None, bits=True, hard=True, counts=True,
                member=True, workspace=None):
    """one mpqe_kg_answers_mixed call -> dict(answers [Q, out_words], hard, counts [2, Q], target [Q], member [Q], err);
    the outputs not asked for are None and their buffers must be untouched"""
    be = world.be
    Q = records.shape[0]
    Wmax = K._words(int(world.mode_rows.max()))
    out_words = Wmax + extra_words
    d_rec = K._at(be, records.astype(np.int64), 8)
    d_probe = None if probe is None else K._at(be, np.asarray(probe, dtype=np.int64), 8)
    M = len(world.mode_rows)
    need = be.lib.mpqe_kg_mixed_workspace_bytes(Q, world.mode_rows.ctypes.data, M, flags)
    assert need >= 256
    ws = K._workspace(be, rng, need, 4) if workspace is None else workspace
    err = be.zeros((1,), np.int32)
    bufs = {'answers': K._fenced(be, rng, Q * out_words), 'hard': K._fenced(be, rng, Q * out_words),
            'counts': K._fenced(be, rng, 2 * Q, item=8), 'target': K._fenced(be, rng, Q), 'member': K._fenced(be, rng, Q)}
    use = {'answers': bits, 'hard': bits and hard, 'counts': counts, 'target': True, 'member': member}
    ptr = {k: be.ptr(bufs[k][1]) if use[k] else None for k in bufs}
    be.check(be.lib.mpqe_kg_answers_mixed(be.ptr(world.table), world.mode_rows.ctypes.data, M, _capi.QUERY_TYPE_IDS[qt],
                                          be.ptr(d_rec), Q, be.ptr(d_probe), ptr['answers'], ptr['hard'], out_words,
                                          ptr['counts'], ptr['target'], ptr['member'], flags, be.ptr(ws), need, be.ptr(err),
                                          be.stream), 'mpqe_kg_answers_mixed')
    sizes = {'answers': Q * out_words, 'hard': Q * out_words, 'counts': 2 * Q, 'target': Q, 'member': Q}
    out = {'err': int(be.get(err)[0])}
    for k, (buf, view, before) in bufs.items():
        K._guards_kept(be, buf, before, sizes[k], k)
        if not use[k]:
            np.testing.assert_array_equal(be.get(buf), before, err_msg='%s = NULL, yet its buffer changed' % k)
            out[k] = None
        else:
            out[k] = be.get(view).copy()
    for k in ('answers', 'hard'):
        if out[k] is not None:
            out[k] = out[k].view(np.uint32).reshape(Q, out_words)
    if out['counts'] is not None:
        out['counts'] = out['counts'].reshape(2, Q)
    np.testing.assert_array_equal(be.get(d_rec), records)                           # (read only)
    K._guards_kept(be, world.table_buf, world.table_before, world.table_need // 8, 'the table')
    return out


def _expected(world, qt, records, out_words, probe=None, empty=()):
    """the oracle's outputs; the queries in `empty` (and those of status 0) produce nothing"""
    Q = records.shape[0]
    a, h = np.zeros((Q, out_words), dtype=np.uint32), np.zeros((Q, out_words), dtype=np.uint32)
    counts, target, member = np.zeros((2, Q), dtype=np.int64), np.full(Q, -1, dtype=np.int32), np.zeros(Q, dtype=np.int32)
    for q, rec in enumerate(records):
        if rec[0] == 0 or q in empty:
            continue
        both, hard, mode = world.sets_of(qt, rec)
        n = int(world.mode_rows[mode])
        a[q, :K._words(n)], h[q, :K._words(n)] = K._bitmap(both, n), K._bitmap(hard, n)
        counts[:, q], target[q] = (len(both), len(hard)), mode
        member[q] = int((rec[1] if probe is None else probe[q]) in both)
    return a, h, counts, target, member


def _check(got, want, what):
    for k, w in zip(('answers', 'hard', 'counts', 'target', 'member'), want):
        if got[k] is not None:
            np.testing.assert_array_equal(got[k], w, err_msg='%s, %s' % (k, what))


# ---------------------------------------------------------------------------------------------- all seven types
@pytest.mark.parametrize('qt', TYPES)
def test_answers_of_mixed_formulas(be, qt):
    """Modes of 1, 33 and 65 rows (words end at 31 | 32 | 33 and 64 | 65), fourteen relations. Every query of the batch has
    another relation tuple, the target modes are mixed. Both homes of the working bitmaps; the per-formula kernel on each
    query alone gives the same words."""
    world = _world(be)
    rng = np.random.RandomState(200 + TYPES.index(qt))
    Q = 8 if qt == '1-chain' else 24
    records = world.random_records(qt, Q, rng)
    n_e = len(PARENT[qt])
    assert len(set(map(tuple, records[:, 2:2 + 3 * n_e:3]))) == Q
    Wmax = K._words(65)
    want = _expected(world, qt, records, Wmax)
    assert len(set(want[3].tolist())) > 1 and want[2][0].max() > 0 and (want[4] == 1).any()
    if 'inter' in qt:
        assert want[2][1].max() > 0
    homes = []
    for flags in (0, _capi.KG_GLOBAL_BITS):
        got = _mixed_call(world, qt, records, rng, flags)
        _check(got, want, 'bitmaps in %s' % ('the workspace' if flags else 'LDS'))
        assert got['err'] == 0
        homes.append(got)
    for k in ('answers', 'hard', 'counts', 'target', 'member'):
        np.testing.assert_array_equal(homes[0][k], homes[1][k])
    for q, rec in enumerate(records):
        a, h, c = world.per_formula(qt, rec, rng)
        W = a.shape[0]
        np.testing.assert_array_equal(homes[0]['answers'][q, :W], a)
        np.testing.assert_array_equal(homes[0]['hard'][q, :W], h)
        np.testing.assert_array_equal(homes[0]['counts'][:, q], c)
        assert not homes[0]['answers'][q, W:].any() and not homes[0]['hard'][q, W:].any()


def test_probe_rows(be):
    """member follows probe_rows where given: rows in the set, outside it, and outside the mode (0, no flag)"""
    world = _world(be)
    rng = np.random.RandomState(5)
    records = world.random_records('2-inter', 12, rng)
    probe = rng.randint(0, 65, size=12)
    probe[0], probe[1] = -1, 65
    want = _expected(world, '2-inter', records, K._words(65), probe=probe)
    got = _mixed_call(world, '2-inter', records, rng, probe=probe)
    _check(got, want, 'probe rows')
    assert got['err'] == 0


# ---------------------------------------------------------------------------------------------- the row stride
@pytest.mark.parametrize('qt', ['2-chain', '3-chain_inter'])
def test_out_words_above_the_widest_mode(be, qt):
    """out_words = W + 3: every word at or above a query's own W is 0 (the buffers start as random bits), guards kept"""
    world = _world(be)
    rng = np.random.RandomState(31)
    records = world.random_records(qt, 9, rng)
    want = _expected(world, qt, records, K._words(65) + 3)
    for flags in (0, _capi.KG_GLOBAL_BITS):
        got = _mixed_call(world, qt, records, rng, flags, extra_words=3)
        _check(got, want, 'stride W + 3')
        assert got['err'] == 0


# ---------------------------------------------------------------------------------------------- one malformed query
LONE = [(1, 2, 'lone', {r: [r, 2 * r] for r in range(33)})]
KINDS = ['status 0', 'anchor n', 'anchor -1', 'relation -1', 'relation R', 'no reverse', 'modes', 'offset', 'row']


# per query type a good record whose LEAF edge (the last anchor's) runs mode 1 -> mode 2 along a relation to choose:
# (source row, relation name or None for that one, destination row) per edge; e: mode 1 -> 1, g: mode 1 -> 2
BASE = {'2-chain': [(3, 'e', 1), (1, None, 7)], '2-inter': [(3, 'g', 7), (3, None, 7)],
        '3-chain_inter': [(3, 'e', 1), (1, 'g', 7), (1, None, 7)]}


def _spoil(world, qt, good, kind):
    """a record of `kind`: from a good one of the batch, or (the kinds that need a certain relation) from BASE"""
    rec = good.copy()
    n_e = len(PARENT[qt])
    leaf = ANCHOR_EDGES[qt][-1]
    R = len(world.names)
    if kind == 'status 0':
        rec[0] = 0
    elif kind == 'anchor n':
        rec[3 + 3 * leaf] = world.mode_rows[world.dst[rec[2 + 3 * leaf]]]
    elif kind == 'anchor -1':
        rec[3 + 3 * leaf] = -1
    elif kind == 'relation -1':
        rec[2 + 3 * (n_e - 1)] = -1
    elif kind == 'relation R':
        rec[2] = R
    else:
        name = {'no reverse': 'lone', 'modes': 'g', 'offset': 'z', 'row': 'z'}[kind]
        for e, (x, rel, y) in enumerate(BASE[qt]):
            m = 'm2' if e == leaf or rel == 'g' else 'm1'
            rec[1 + 3 * e:4 + 3 * e] = (x, world.index[('m1', rel or name, m)], y)
        if kind == 'modes':
            # 2-chain, 3-chain_inter: the hop along edge 0 leaves mode 2, the frontier is in mode 1; 2-inter: the branch of
            # edge 0 ends in mode 0, the other in mode 1
            rec[2] = world.index[('m0', 'c', 'm2')] if qt == '2-inter' else world.index[('m2', 'f', 'm2')]
        if kind in ('offset', 'row'):
            rec[3 + 3 * leaf] = 9
    return rec


@pytest.mark.parametrize('qt', ['2-chain', '2-inter', '3-chain_inter'])
def test_one_malformed_query_among_good_ones(be, qt):
    """One query of each kind between six good ones: its sets are empty and every word of them written, BAD_INDEX is raised
    exactly when the kind asks for it (a status of 0 does not), the neighbours' words are those of the clean batch.
    'offset' / 'row': relation z's inverse (mode 2 -> mode 1, used by no other query) has a corrupt offset behind row 9,
    resp. a row of 33 in row 9's list; the spoilt record's anchor is row 9 of that CSR."""
    z = (1, 2, 'z', {r: [9] for r in range(4)})
    world = MixedWorld(be, ROWS, _pairs(np.random.RandomState(23)) + [z], LONE)
    rng = np.random.RandomState(77)
    good = world.random_records(qt, 40, rng)
    good = good[[('z' not in [world.names[r][1] for r in g[2:2 + 3 * len(PARENT[qt]):3]]) for g in good]][:6]
    assert good.shape[0] == 6
    inv = world.index[('m2', 'z', 'm1')]
    d_off, d_rows = world.keep[2 * inv], world.keep[2 * inv + 1]
    edges = int(world.edges[inv])
    assert edges == 4 and be.get(d_off)[9:11].tolist() == [0, 4]
    for kind in KINDS:
        if kind == 'offset':
            _poke(d_off, 10, edges + 5)
        if kind == 'row':
            _poke(d_rows, 2, 33)
        records = np.concatenate([good[:3], _spoil(world, qt, good[0], kind)[None, :], good[3:]])
        want = _expected(world, qt, records, K._words(65), empty={3})
        for flags in (0, _capi.KG_GLOBAL_BITS):
            got = _mixed_call(world, qt, records, rng, flags)
            _check(got, want, kind)
            assert got['err'] == (0 if kind == 'status 0' else BAD_INDEX), kind
        if kind == 'offset':
            _poke(d_off, 10, edges)
        if kind == 'row':
            _poke(d_rows, 2, 2)
    # the record of 'offset' / 'row' on the mended CSR is a good query
    records = _spoil(world, qt, good[0], 'row')[None, :]
    got = _mixed_call(world, qt, records, rng)
    _check(got, _expected(world, qt, records, K._words(65)), 'mended')
    assert got['err'] == 0 and got['target'][0] >= 0


# ---------------------------------------------------------------------------------------------- degree edges
# (source row, relation, destination row) per edge with the last anchor `a`; b_inv: mode 2 -> 1, its hop walks b out of mode 1
HUB = {'1-chain': lambda a: [(0, 'b_inv', a)],
       '2-chain': lambda a: [(0, 'b_inv', 5), (5, 'e', a)],
       '3-inter_chain': lambda a: [(0, 'b_inv', 5), (0, 'b_inv', 5), (5, 'e', a)]}


@pytest.mark.parametrize('qt', ['1-chain', '2-chain', '3-inter_chain'])
def test_hub_row_empty_lists_and_repeats(be, qt):
    """Row 5 of mode 1 has a list of 1 000 entries in relation b (repeats: 65 rows to land on; its inverse's lists name row 5
    again and again), row 6 has none. 1-chain: the anchor's own list (the workgroup strides over it); 2-chain and
    3-inter_chain: rows 5 and 6 are in the frontier that e's hop from rows 6 / 8 / 5 leaves (a wave strides)."""
    world = _world(be, hub=True)
    b = world.index[('m1', 'b', 'm2')]
    name = {'b_inv': ('m2', 'b', 'm1'), 'e': ('m1', 'e', 'm1')}
    assert len(world.relations[b][2][5]) == 1000 and 6 not in world.relations[b][2]
    e_lists = world.lists[name['e']]
    assert 5 in e_lists[6] and 5 in e_lists[8] and 6 in e_lists[5]
    rng = np.random.RandomState(41)
    records = [r for r in world.random_records(qt, 5, rng)]
    for a in (5, 6, 8):
        rec = np.full(_capi.KG_QUERY_INTS, -1, dtype=np.int64)
        rec[0] = 1
        for e, (x, rel, y) in enumerate(HUB[qt](a)):
            rec[1 + 3 * e:4 + 3 * e] = (x, world.index[name[rel]], y)
        records.append(rec)
    records = np.stack(records)
    want = _expected(world, qt, records, K._words(65))
    for flags in (0, _capi.KG_GLOBAL_BITS):
        got = _mixed_call(world, qt, records, rng, flags)
        _check(got, want, 'hub')
        assert got['err'] == 0
    hub = len(set(world.relations[b][2][5]))
    assert hub > 60
    if qt == '1-chain':
        assert want[2][0][-3:].tolist() == [hub, 0, len(set(world.relations[b][2].get(8, ())))]
    else:
        assert (want[2][0][-2:] >= (hub if qt == '2-chain' else 1)).all()         # (anchors 6 and 8: row 5 is in the frontier)


# ---------------------------------------------------------------------------------------------- no bitmap leaves
@pytest.mark.parametrize('qt', ['3-inter', '3-chain_inter', '2-chain'])
def test_call_without_bitmaps(be, qt):
    """answers = hard = NULL (MPQE_KG_COUNT_HARD): counts, target_mode and member are the full call's; without the flag
    |hard| is 0 and the rest unchanged; counts and member may be NULL too"""
    world = _world(be)
    rng = np.random.RandomState(9)
    records = world.random_records(qt, 10, rng)
    records[4, 0] = 0
    full = _mixed_call(world, qt, records, rng)
    assert full['err'] == 0
    for home in (0, _capi.KG_GLOBAL_BITS):
        bare = _mixed_call(world, qt, records, rng, home | _capi.KG_COUNT_HARD, bits=False)
        for k in ('counts', 'target', 'member'):
            np.testing.assert_array_equal(bare[k], full[k], err_msg=k)
        plain = _mixed_call(world, qt, records, rng, home, bits=False)
        np.testing.assert_array_equal(plain['counts'][0], full['counts'][0])
        assert not plain['counts'][1].any()
        np.testing.assert_array_equal(plain['member'], full['member'])
        least = _mixed_call(world, qt, records, rng, home, bits=False, counts=False, member=False)
        np.testing.assert_array_equal(least['target'], full['target'])
        answers_only = _mixed_call(world, qt, records, rng, home, hard=False)
        np.testing.assert_array_equal(answers_only['answers'], full['answers'])
        np.testing.assert_array_equal(answers_only['counts'][0], full['counts'][0])


# ---------------------------------------------------------------------------------------------- sizes, refusals
def test_size_query_and_workspace(be):
    """Q == 0 launches nothing (made-up pointers); a workspace one byte short: MPQE_ERR_WORKSPACE and no output written; a
    workspace of exactly the size asked, fenced: the oracle's words and the fences intact"""
    from tests.fenced import assert_fence_intact, fenced_bytes
    world = _world(be)
    lib, M, fake = be.lib, len(world.mode_rows), 0x10000
    rows = world.mode_rows.ctypes.data
    G = _capi.KG_GLOBAL_BITS
    assert lib.mpqe_kg_mixed_workspace_bytes(5, rows, M, 0) == 256
    assert lib.mpqe_kg_mixed_workspace_bytes(5, rows, M, G) == 5 * 4 * 3 * 4 + 16 + 256         # (240 -> 256) + 256
    assert lib.mpqe_kg_mixed_workspace_bytes(-1, rows, M, 0) == 0 and lib.mpqe_kg_mixed_workspace_bytes(5, rows, 17, 0) == 0
    assert lib.mpqe_kg_table_bytes(0, 3) == 0 and lib.mpqe_kg_table_bytes(4097, 3) == 0 and lib.mpqe_kg_table_bytes(3, 17) == 0
    assert lib.mpqe_kg_table_bytes(4096, 16) >= 4096 * 48

    def call(table=fake, qt=3, rec=fake, Q=5, answers=fake, hard=fake, words=3, target=fake, flags=G, ws=fake, wb=1 << 20):
        return lib.mpqe_kg_answers_mixed(table, rows, M, qt, rec, Q, None, answers, hard, words, fake, target, fake, flags, ws,
                                         wb, None, None)
    assert call(Q=0) == OK and call(Q=0, table=None, rec=None, target=None, ws=None, wb=0) == OK
    assert call(qt=7) == INVALID and call(qt=-1) == INVALID and call(Q=-1) == INVALID and call(flags=4) == INVALID
    assert call(words=2) == INVALID and call(table=None) == INVALID and call(rec=None) == INVALID
    assert call(target=None) == INVALID and call(ws=None) == INVALID and call(ws=fake + 2) == INVALID
    assert call(table=fake + 4) == INVALID
    need = lib.mpqe_kg_mixed_workspace_bytes(5, rows, M, G)
    assert call(wb=need - 1) == WORKSPACE and call(wb=255, flags=0) == WORKSPACE

    rng = np.random.RandomState(3)
    records = world.random_records('3-inter_chain', 5, rng)
    want = _expected(world, '3-inter_chain', records, 3)
    for fill in ('nan', 'ones'):
        ws = fenced_bytes(be, need, fill, align=256, misalign=4)
        got = _mixed_call(world, '3-inter_chain', records, rng, G, workspace=ws)
        _check(got, want, 'exact workspace')
        assert got['err'] == 0
        assert_fence_intact(be, ws, 'the mixed workspace')
    # one byte short, real operands: refused before anything is written
    d_rec = K._at(be, records, 8)
    buf, view, before = K._fenced(be, rng, 5 * 3)
    st = lib.mpqe_kg_answers_mixed(be.ptr(world.table), rows, M, 5, be.ptr(d_rec), 5, None, be.ptr(view), None, 3, None,
                                   be.ptr(view), None, G, be.ptr(ws), need - 1, None, be.stream)
    assert st == WORKSPACE
    np.testing.assert_array_equal(be.get(buf), before)

    def build(offs=world.offs, src=world.src, rev=world.reverse, R=len(world.names), table=fake, tb=1 << 20):
        return lib.mpqe_kg_table_build(offs, world.rows, world.edges, src.ctypes.data, world.dst.ctypes.data, rev.ctypes.data,
                                       R, rows, world.valid_ptrs, world.row_id_ptrs, M, table, tb, None)
    assert build(offs=None) == INVALID and build(table=None) == INVALID and build(table=fake + 4) == INVALID
    assert build(R=0) == INVALID and build(tb=world.table_need - 1) == WORKSPACE
    assert build(src=np.full(len(world.names), 3, dtype=np.int32)) == INVALID
    assert build(rev=np.full(len(world.names), len(world.names), dtype=np.int32)) == INVALID


def test_same_call_twice_gives_the_same_bits(be):
    world = _world(be)
    rng = np.random.RandomState(50)
    records = world.random_records('3-chain_inter', 17, rng)
    one = _mixed_call(world, '3-chain_inter', records, rng, _capi.KG_GLOBAL_BITS)
    two = _mixed_call(world, '3-chain_inter', records, rng, _capi.KG_GLOBAL_BITS)
    assert all(np.array_equal(one[k], two[k]) for k in ('answers', 'hard', 'counts', 'target', 'member')) and one['err'] == 0


# ---------------------------------------------------------------------------------------------- mpqe_kg_sample_rows_mixed
SAMPLE_ROWS = [1, 33, 65, 2049]


@pytest.fixture(scope='module')
def sample_world(be):
    """four modes of 1, 33, 65 and 2 049 rows (`valid` with holes, row ids 1000 m + 7 row) and one relation without an edge"""
    return MixedWorld(be, SAMPLE_ROWS, [(0, 0, 'none', {})])


def _raw_sets(rng, Q, stride):
    """random bits [Q, 32 stride] -- also behind every mode's rows: those name no row; query 1 empty, query 2 full"""
    raw = rng.rand(Q, 32 * stride) < 0.4
    raw[1], raw[2] = False, True
    raw[3] = rng.rand(32 * stride) < 0.02
    return raw


def _selected(world, raw, mode, select):
    n = SAMPLE_ROWS[mode]
    member = raw[:n]
    return np.nonzero(member if select == _capi.KG_ROWS_SET else ~member & world.is_valid[mode])[0]


def _sample_mixed(world, rng, bits, stride, modes, select, lengths, k, seed, q_base=0, slack=1, rows=True, ids=True):
    """-> (offsets, rows [total] or None, ids [total] or None, error word); outputs fenced, slack kept"""
    be = world.be
    Q = bits.shape[0]
    off = np.zeros(Q + 1, dtype=np.int64)
    off[1:] = np.cumsum(lengths)
    total = int(off[-1])
    d_bits, d_modes, d_off = K._at(be, bits.view(np.int32), 4), K._at(be, modes.astype(np.int32), 4), K._at(be, off, 8)
    r_buf, r_view, r_before = K._fenced(be, rng, total + slack + 1, item=8)
    i_buf, i_view, i_before = K._fenced(be, rng, total + slack + 1, item=8)
    err = be.zeros((1,), np.int32)
    be.check(be.lib.mpqe_kg_sample_rows_mixed(be.ptr(world.table), world.mode_rows.ctypes.data, len(world.mode_rows),
                                              be.ptr(d_bits), stride, be.ptr(d_modes), Q, q_base, select, be.ptr(d_off),
                                              be.ptr(r_view) if rows else None, be.ptr(i_view) if ids else None,
                                              total + slack, k, seed, be.ptr(err), be.stream), 'mpqe_kg_sample_rows_mixed')
    out = []
    for use, (buf, view, before) in ((rows, (r_buf, r_view, r_before)), (ids, (i_buf, i_view, i_before))):
        K._guards_kept(be, buf, before, total + slack + 1, 'rows_out / ids_out')
        got = be.get(view)
        np.testing.assert_array_equal(got[total:], before[K.GUARD + total:K.GUARD + total + slack + 1], err_msg='slack')
        if not use:
            np.testing.assert_array_equal(be.get(buf), before, err_msg='a NULL output was written')
        out.append(got[:total].copy() if use else None)
    return off, out[0], out[1], int(be.get(err)[0])


@pytest.mark.parametrize('select', [_capi.KG_ROWS_SET, _capi.KG_ROWS_COMPLEMENT])
@pytest.mark.parametrize('k', [3, 100])
def test_sample_rows_mixed(be, sample_world, k, select):
    """20 queries over modes of 1, 33, 65 and 2 049 rows and two of mode -1, bitmaps 67 words apart (65 + 2). c <= k: all
    members ascending; c > k: the restated draw, keyed by (seed, q_base + q). Equal to mpqe_kg_sample_rows called per mode
    on the same batch; ids_out = the table's row ids of rows_out; a batch split in two with q_base gives the unsplit lists."""
    world = sample_world
    rng = np.random.RandomState(17 * k + select)
    Q, stride, seed = 22, K._words(2049) + 2, 1234567
    modes = np.array([0, 1, 2, 3] * 5 + [-1, -1])
    rng.shuffle(modes[4:])
    raw = _raw_sets(rng, Q, stride)
    bits = np.packbits(raw, axis=1, bitorder='little').view(np.uint32).reshape(Q, stride)
    chosen = [_selected(world, raw[q], modes[q], select) if modes[q] >= 0 else np.zeros(0, np.int64) for q in range(Q)]
    lengths = np.array([min(len(c), k) for c in chosen])
    assert any(len(c) > k for c in chosen) and (k < 100 or any(0 < len(c) < k for c in chosen))
    off, rows, ids, err = _sample_mixed(world, rng, bits, stride, modes, select, lengths, k, seed, q_base=40)
    assert err == 0
    for q in range(Q):
        mine = rows[off[q]:off[q + 1]]
        np.testing.assert_array_equal(mine, oracle.sample_rows(chosen[q].tolist(), k, seed, 40 + q), err_msg='query %d' % q)
        if modes[q] >= 0:
            np.testing.assert_array_equal(ids[off[q]:off[q + 1]], world.row_ids[modes[q]][mine])
    # each output alone
    only_rows = _sample_mixed(world, rng, bits, stride, modes, select, lengths, k, seed, q_base=40, ids=False)
    only_ids = _sample_mixed(world, rng, bits, stride, modes, select, lengths, k, seed, q_base=40, rows=False)
    np.testing.assert_array_equal(only_rows[1], rows)
    np.testing.assert_array_equal(only_ids[2], ids)
    # mpqe_kg_sample_rows per mode on the same batch (q_base 0: its key is the position alone)
    off0, rows0, _, err = _sample_mixed(world, rng, bits, stride, modes, select, lengths, k, seed)
    assert err == 0
    for m, n in enumerate(SAMPLE_ROWS):
        W = K._words(n)
        sel = [_selected(world, raw[q], m, select) for q in range(Q)]
        valid = T._pack(world.is_valid[m][None, :])[0]
        off_m, rows_m, err = T._sample_rows(be, rng, np.ascontiguousarray(bits[:, :W]), n, valid, select,
                                            [min(len(s), k) for s in sel], k, seed)
        assert err == 0
        for q in np.nonzero(modes == m)[0]:
            np.testing.assert_array_equal(rows0[off0[q]:off0[q + 1]], rows_m[off_m[q]:off_m[q + 1]], err_msg='mode %d' % m)
    # the batch in two halves
    cut = 9
    first = _sample_mixed(world, rng, bits[:cut], stride, modes[:cut], select, lengths[:cut], k, seed, q_base=40)
    second = _sample_mixed(world, rng, bits[cut:], stride, modes[cut:], select, lengths[cut:], k, seed, q_base=40 + cut)
    assert first[3] == 0 and second[3] == 0
    np.testing.assert_array_equal(np.concatenate([first[1], second[1]]), rows)
    np.testing.assert_array_equal(np.concatenate([first[2], second[2]]), ids)


def test_sample_rows_mixed_with_wrong_segments(be, sample_world):
    """a segment one slot shorter / longer than min(k, c), a query of mode -1 with a slot, a mode of 4: MPQE_FLAG_BAD_INDEX,
    nothing lands outside a query's own segment (_sample_mixed checks guards and slack), the other queries are exact"""
    world = sample_world
    rng = np.random.RandomState(4)
    stride, k, seed = K._words(2049), 4, 5
    modes = np.array([1, 2, 3, -1, 2])
    raw = rng.rand(5, 32 * stride) < 0.5
    bits = np.packbits(raw, axis=1, bitorder='little').view(np.uint32).reshape(5, stride)
    chosen = [_selected(world, raw[q], modes[q], _capi.KG_ROWS_SET) if modes[q] >= 0 else [] for q in range(5)]
    true = np.array([min(len(c), k) for c in chosen])
    for delta, bad_mode in (([0, -1, 1, 0, 0], None), ([0, 0, 0, 1, 0], None), ([0, 0, 0, 0, 0], 4), ([0, 0, 0, 0, 0], -2)):
        use = modes.copy()
        if bad_mode is not None:
            use[1] = bad_mode
        lengths = true + np.array(delta)
        off, rows, ids, err = _sample_mixed(world, rng, bits, stride, use, _capi.KG_ROWS_SET, lengths, k, seed)
        assert err == BAD_INDEX
        for q in range(5):
            if modes[q] < 0 or (bad_mode is not None and q == 1):
                continue
            want = oracle.sample_rows(list(chosen[q]), k, seed, q)
            m = min(len(want), int(lengths[q]))
            np.testing.assert_array_equal(rows[off[q]:off[q] + m], want[:m])
    assert _sample_mixed(world, rng, bits, stride, modes, _capi.KG_ROWS_SET, true, k, seed)[3] == 0


def test_sample_rows_mixed_refuses_before_any_launch(be, sample_world):
    world = sample_world
    lib, fake, rows = be.lib, 0x10000, world.mode_rows.ctypes.data

    def call(table=fake, M=4, bits=fake, stride=65, modes=fake, Q=5, q_base=0, select=0, offsets=fake, out=fake, ids=None,
             cap=10, k=3):
        return lib.mpqe_kg_sample_rows_mixed(table, rows, M, bits, stride, modes, Q, q_base, select, offsets, out, ids, cap, k,
                                             1, None, None)
    assert call(Q=0) == OK and call(select=2) == INVALID and call(k=0) == INVALID and call(q_base=-1) == INVALID
    assert call(k=_capi.KG_SAMPLE_MAX_K + 1) == -2 and call(stride=64) == INVALID and call(M=0) == INVALID
    assert call(table=None) == INVALID and call(bits=None) == INVALID and call(modes=None) == INVALID
    assert call(offsets=None) == INVALID and call(out=None) == INVALID and call(out=None, ids=fake, Q=0) == OK
    assert call(Q=-1) == INVALID and call(cap=-1) == INVALID
