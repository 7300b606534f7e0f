"""csrc/kg.hip through the C ABI (mpqe_kg_answers, mpqe_kg_rows), on the host emulator and (gpu) on the real library, against
the set oracle of tests/kg_oracle.py. Every comparison is exact -- whole words, so a bit at or above a mode's row count
fails it.

Every mpqe_kg_answers call here (_answers) runs BOTH homes of the working bitmaps (LDS, and MPQE_KG_GLOBAL_BITS: the
workspace) and wants identical words; workspace and outputs hold random bits when a call starts; every output sits between
guard words that must keep theirs; the 4-byte operands (bitmaps, valid) start 4 bytes past a 16-byte boundary, the int64
ones (anchors, CSR arrays, counts, offsets, row lists) 8 bytes past one -- their own alignment, and no more."""
import ctypes

import numpy as np
import pytest

from mpqe_amd import _capi
from mpqe_amd.kg import kg_programme
from tests import kg_oracle

BAD_INDEX = _capi.FLAG_BAD_INDEX
GUARD = 3               # words on either side of an output


@pytest.fixture(scope='module', params=['emu', pytest.param('hip', marks=pytest.mark.gpu)])
def be(request):
    from tests import kernel_backend
    return kernel_backend.EmuBackend() if request.param == 'emu' else kernel_backend.HipBackend()


def _at(be, host, misalign=0):
    """`host` on the backend, its first byte `misalign` bytes past a 256-byte boundary (a view of a larger allocation)"""
    host = np.ascontiguousarray(host)
    item = host.dtype.itemsize
    assert misalign % item == 0 and host.size > 0
    raw = be.zeros(host.size + (512 + misalign) // item, host.dtype)
    skip = ((-be.ptr(raw)) % 256 + misalign) // item
    view = raw[skip:skip + host.size]
    if be.name == 'emu':
        view[:] = host.ravel()
    else:
        view.copy_(be.put(host.ravel()))
    assert be.ptr(view) % 256 == misalign
    return view.reshape(host.shape)


def _garbage(rng, words):
    return rng.randint(-2 ** 31, 2 ** 31 - 1, size=int(words)).astype(np.int32)


def _workspace(be, rng, need, misalign):
    """The workspace of one call: random bits, `misalign` bytes past a 256-byte boundary, a word more than asked. (One place,
    so that tests/test_workspace_bounds.py can put an exact, fenced buffer there instead.)"""
    return _at(be, _garbage(rng, need // 4 + 1), misalign)


def _fenced(be, rng, words, item=4):
    """-> (the whole buffer, the view of `words` elements behind GUARD guard elements, the buffer's bits on the host): random
    bits everywhere; the view's first byte is 4 (int32) / 8 (int64) bytes past a 16-byte boundary"""
    if item == 4:
        host = _garbage(rng, words + 2 * GUARD)
        buf = _at(be, host, misalign=16 + 4 - 4 * GUARD)
    else:
        host = _garbage(rng, 2 * (words + 2 * GUARD)).view(np.int64)
        buf = _at(be, host, misalign=32 + 8 - 8 * GUARD)
    view = buf[GUARD:GUARD + words]
    assert be.ptr(view) % 16 == item
    return buf, view, host.copy()


def _guards_kept(be, buf, before, words, what):
    after = be.get(buf)
    np.testing.assert_array_equal(after[:GUARD], before[:GUARD], err_msg='guard in front of ' + what)
    np.testing.assert_array_equal(after[GUARD + words:], before[GUARD + words:], err_msg='guard behind ' + what)


def _words(n):
    return (n + 31) // 32


def _bitmap(rows, n):
    flags = np.zeros(_words(n) * 32, dtype=np.uint8)
    flags[sorted(rows)] = 1
    return np.packbits(flags, bitorder='little').view(np.uint32)


class World(object):
    """modes: their row counts; relations: (source mode, destination mode, {row: [rows]}) -- lists as given (unsorted,
    repeats). The CSR arrays live on the backend, 8 bytes past a 16-byte boundary."""

    def __init__(self, be, mode_rows, relations):
        self.be, self.mode_rows, self.relations = be, np.asarray(mode_rows, dtype=np.int64), relations
        self.keep, offs, rows, edges = [], [], [], []
        for src, dst, lists in relations:
            n = int(self.mode_rows[src])
            off = np.zeros(n + 1, dtype=np.int64)
            off[1:] = np.cumsum([len(lists.get(r, ())) for r in range(n)])
            flat = np.array([x for r in range(n) for x in lists.get(r, ())] + [-1], dtype=np.int64)   # (+ one: never empty)
            d_off, d_rows = _at(be, off, 8), _at(be, flat, 8)
            self.keep += [d_off, d_rows]
            offs.append(be.ptr(d_off))
            rows.append(be.ptr(d_rows))
            edges.append(int(off[-1]))
        R = len(relations)
        self.offs, self.rows = (ctypes.c_void_p * R)(*offs), (ctypes.c_void_p * R)(*rows)
        self.edges = (ctypes.c_int64 * R)(*edges)

    def programme(self, branches, tail):
        """branches: [(anchor mode, [relation index])], tail: [relation index] -> (programme, target mode)"""
        dst = lambda r: self.relations[r][1]                               # noqa: E731
        for mode, steps in branches:
            for r in steps:
                assert self.relations[r][0] == mode
                mode = dst(r)
        for r in tail:
            assert self.relations[r][0] == mode
            mode = dst(r)
        prog = kg_programme([(m, [(r, dst(r)) for r in steps]) for m, steps in branches], [(r, dst(r)) for r in tail], mode)
        return np.ascontiguousarray(prog), mode

    def oracle(self, branches, tail, anchors):
        """-> per query (answers, hard) as sets of rows"""
        out = []
        for q in range(anchors.shape[1]):
            both, some = kg_oracle.programme_sets([[self.relations[r][2] for r in steps] for _, steps in branches],
                                                  [self.relations[r][2] for r in tail], [int(a) for a in anchors[:, q]])
            out.append((both, some - both))
        return out


def _call(world, prog, anchors, n_out, rng, flags, hard=True, counts=True):
    """one mpqe_kg_answers call -> (answers [Q, W] uint32, hard or None, counts [2, Q] or None, the error word)"""
    be = world.be
    Q, W = anchors.shape[1], _words(n_out)
    d_anchors = _at(be, anchors.astype(np.int64), 8)
    need = be.lib.mpqe_kg_workspace_bytes(prog.ctypes.data, Q, world.mode_rows.ctypes.data, len(world.mode_rows), flags)
    assert need >= 256
    ws = _workspace(be, rng, need, 4)
    err = be.zeros((1,), np.int32)
    a_buf, a_view, a_before = _fenced(be, rng, Q * W)
    h_buf, h_view, h_before = _fenced(be, rng, Q * W)
    c_buf, c_view, c_before = _fenced(be, rng, 2 * Q, item=8)
    be.check(be.lib.mpqe_kg_answers(prog.ctypes.data, world.offs, world.rows, world.edges, len(world.relations),
                                    world.mode_rows.ctypes.data, len(world.mode_rows), be.ptr(d_anchors), Q, be.ptr(a_view),
                                    be.ptr(h_view) if hard else None, be.ptr(c_view) if counts else None, flags, be.ptr(ws),
                                    need, be.ptr(err), be.stream), 'mpqe_kg_answers')
    _guards_kept(be, a_buf, a_before, Q * W, 'answers')
    _guards_kept(be, h_buf, h_before, Q * W, 'hard')
    _guards_kept(be, c_buf, c_before, 2 * Q, 'counts')
    got_a = be.get(a_view).view(np.uint32).reshape(Q, W).copy()
    got_h = be.get(h_view).view(np.uint32).reshape(Q, W).copy()
    got_c = be.get(c_view).reshape(2, Q).copy()
    if not hard:
        np.testing.assert_array_equal(be.get(h_buf), h_before, err_msg='hard = NULL, yet its buffer changed')
    if not counts:
        np.testing.assert_array_equal(be.get(c_buf), c_before, err_msg='counts = NULL, yet its buffer changed')
    return got_a, got_h if hard else None, got_c if counts else None, int(be.get(err)[0])


def _answers(world, branches, tail, anchors, seed, want_flags=0):
    """Both homes of the bitmaps against the oracle (queries whose anchors are outside their mode: empty sets). -> the
    oracle's sets."""
    rng = np.random.RandomState(seed)
    anchors = np.asarray(anchors, dtype=np.int64).reshape(len(branches), -1)
    prog, target = world.programme(branches, tail)
    n_out = int(world.mode_rows[target])
    inside = np.array([all(0 <= anchors[b, q] < world.mode_rows[branches[b][0]] for b in range(len(branches)))
                       for q in range(anchors.shape[1])])
    want = world.oracle(branches, tail, np.where(inside[None, :], anchors, 0))
    want = [w if ok else (set(), set()) for w, ok in zip(want, inside)]
    want_a = np.stack([_bitmap(w[0], n_out) for w in want])
    want_h = np.stack([_bitmap(w[1], n_out) for w in want])
    want_c = np.array([[len(w[0]) for w in want], [len(w[1]) for w in want]], dtype=np.int64)
    for flags in (0, _capi.KG_GLOBAL_BITS):
        got_a, got_h, got_c, err = _call(world, prog, anchors, n_out, rng, flags)
        what = 'bitmaps in %s' % ('the workspace' if flags else 'LDS')
        np.testing.assert_array_equal(got_a, want_a, err_msg='answers, ' + what)
        np.testing.assert_array_equal(got_h, want_h, err_msg='hard, ' + what)
        np.testing.assert_array_equal(got_c, want_c, err_msg='counts, ' + what)
        assert err == want_flags, what
    return want


def _random_lists(rng, n_src, n_dst, max_degree):
    """lists of 0 .. max_degree rows, with repeats, unsorted; some rows have none"""
    return {r: rng.randint(0, n_dst, size=rng.randint(0, max_degree + 1)).tolist() for r in range(n_src) if rng.rand() < 0.8}


# ---------------------------------------------------------------------------------------------- word edges
@pytest.mark.parametrize('n', [1, 31, 32, 33, 64, 65, 2049])
def test_word_edges(be, n):
    """A mode of n rows onto itself: one hop and two. Row n - 1 (the last bit that may be set) is in a list and is an anchor;
    the words are compared whole, so a bit at or above n fails."""
    rng = np.random.RandomState(n)
    lists = _random_lists(rng, n, n, 4)
    lists[n - 1] = [n - 1, 0, n - 1]
    lists[0] = [n - 1] + lists.get(0, [])
    world = World(be, [n], [(0, 0, lists)])
    anchors = [0, n - 1, int(rng.randint(n))]
    one = _answers(world, [(0, [0])], [], anchors, 1)
    two = _answers(world, [(0, [0, 0])], [], anchors, 2)
    assert n - 1 in one[0][0] and n - 1 in one[1][0] and n - 1 in two[1][0]
    assert all(not hard for _, hard in one + two)                   # one branch: no hard negatives


def test_chain_through_modes_of_different_sizes(be):
    """33 -> 2049 -> 31 rows: every hop's bitmap has another width (2, 65 and 1 words); then on through 2049 again"""
    rng = np.random.RandomState(7)
    a = _random_lists(rng, 33, 2049, 40)
    a[32] = [2048, 0, 2047, 2048]
    b = _random_lists(rng, 2049, 31, 3)
    b[2048] = [30]
    c = _random_lists(rng, 31, 2049, 9)
    c[30] = [2048, 2016]
    world = World(be, [33, 2049, 31], [(0, 1, a), (1, 2, b), (2, 1, c)])
    anchors = [32, 0, 17]
    two = _answers(world, [(0, [0, 1])], [], anchors, 3)
    three = _answers(world, [(0, [0, 1, 2])], [], anchors, 4)
    assert 30 in two[0][0] and 2048 in three[0][0]


# ---------------------------------------------------------------------------------------------- list edges
DEGREES = (0, 1, 63, 64, 65, 257, 1025)


def test_list_edges(be):
    """Source rows of degree 0, 1, 63, 64, 65, 257 and 1025: a wave's stride of 64 and a workgroup's of 256, each +- 1, and
    several strides. As the first hop (the workgroup strides over the anchor's list) and as a second hop behind a frontier
    of one bit (a wave strides). Lists are unsorted and repeat rows; the longest holds every row of its mode."""
    rng = np.random.RandomState(11)
    n_dst = 700
    lists = {}
    for r, d in enumerate(DEGREES):
        lists[r] = rng.randint(0, n_dst, size=d).tolist()
    lists[6] = rng.permutation(np.concatenate([np.arange(n_dst), rng.randint(0, n_dst, size=1025 - n_dst)])).tolist()
    assert [len(lists[r]) for r in range(7)] == list(DEGREES) and set(lists[6]) == set(range(n_dst))
    assert len(set(lists[5])) < 257 and lists[5] != sorted(lists[5])
    ident = {r: [r] for r in range(7)}
    world = World(be, [7, n_dst, 7], [(0, 1, lists), (2, 0, ident)])
    first = _answers(world, [(0, [0])], [], list(range(7)), 5)
    second = _answers(world, [(2, [1, 0])], [], list(range(7)), 6)
    assert first == second and [len(a) for a, _ in first][:2] == [0, 1] and len(first[6][0]) == n_dst


# ---------------------------------------------------------------------------------------------- frontier edges
def test_frontier_edges(be):
    """After the first hop the frontier holds 0, 1, 64, 65 and 130 rows (more than the workgroup has waves; bits in one word
    and across words). The empty frontier stays empty through two more hops, and empties the AND with a branch that is not."""
    rng = np.random.RandomState(13)
    sizes = (0, 1, 64, 65, 130)
    first = {r: rng.choice(200, size=s, replace=False).tolist() for r, s in enumerate(sizes)}
    first[2] = list(range(64, 128))                                   # two whole words
    mid, last = _random_lists(rng, 200, 300, 5), _random_lists(rng, 300, 90, 3)
    side = {r: rng.randint(0, 300, size=20).tolist() for r in range(5)}
    world = World(be, [5, 200, 300, 90], [(0, 1, first), (1, 2, mid), (2, 3, last), (0, 2, side)])
    chain = _answers(world, [(0, [0, 1, 2])], [], list(range(5)), 8)
    assert not chain[0][0] and all(chain[q][0] for q in range(2, 5))
    inter = _answers(world, [(0, [3]), (0, [0, 1])], [], [list(range(5)), list(range(5))], 9)
    assert not inter[0][0] and inter[0][1] == set(side[0])          # AND with nothing; the union is the other branch
    tail = _answers(world, [(0, [3]), (0, [0, 1])], [2], [list(range(5)), list(range(5))], 10)
    assert not tail[0][0] and tail[0][1]


# ---------------------------------------------------------------------------------------------- the seven query types
def _seven_world(be):
    """modes of 65, 33 and 100 rows; relations 0 .. 8 = every ordered pair of modes (index 3 * source + destination), random;
    9 and 10: mode 1 -> mode 0 with images in rows < 30 / >= 30 (disjoint sets); 11: relation 9's lists and row 40"""
    rng = np.random.RandomState(17)
    rows = [65, 33, 100]
    rels = [(s, d, _random_lists(rng, rows[s], rows[d], 6)) for s in range(3) for d in range(3)]
    rels.append((1, 0, {r: rng.randint(0, 30, size=4).tolist() for r in range(33)}))
    rels.append((1, 0, {r: rng.randint(30, 65, size=4).tolist() for r in range(33)}))
    rels.append((1, 0, {r: [40] + l[::-1] for r, l in rels[9][2].items()}))
    return World(be, rows, rels)


SEVEN = {            # the programme of each query type: (branches [(anchor mode, [relations])], tail)
    '1-chain': ([(1, [3])], []),
    '2-chain': ([(2, [7, 3])], []),
    '3-chain': ([(0, [2, 7, 3])], []),
    '2-inter': ([(1, [3]), (2, [6])], []),
    '3-inter': ([(1, [3]), (2, [6]), (0, [0])], []),
    '3-inter_chain': ([(1, [3]), (0, [2, 6])], []),
    '3-chain_inter': ([(0, [2]), (1, [5])], [6]),
}


@pytest.mark.parametrize('Q', [1, 3, 17])
@pytest.mark.parametrize('qt', list(SEVEN))
def test_all_seven_query_types(be, qt, Q):
    world = _seven_world(be)
    branches, tail = SEVEN[qt]
    rng = np.random.RandomState(100 + Q)
    anchors = np.stack([rng.randint(0, world.mode_rows[m], size=Q) for m, _ in branches])
    want = _answers(world, branches, tail, anchors, 20 + Q)
    assert len(want) == Q
    if len(branches) == 1:
        assert all(not hard for _, hard in want)                    # chains: all zero
    elif Q == 17:
        assert any(hard for _, hard in want)


def test_same_anchor_thrice_and_disjoint_branches(be):
    world = _seven_world(be)
    have = [r for r in range(33) if world.relations[3][2].get(r)][:3]
    same = _answers(world, [(1, [3]), (1, [3]), (1, [3])], [], [have] * 3, 30)
    assert all(a and not hard for a, hard in same)                  # AND = OR: nothing is hard
    nested = _answers(world, [(1, [9]), (1, [11])], [], [[1, 2, 3], [1, 2, 3]], 33)
    assert all(a and hard == {40} for a, hard in nested)            # one branch inside the other
    nested_tail = _answers(world, [(1, [9]), (1, [11])], [1], [[1, 2, 3], [1, 2, 3]], 34)
    assert any(a for a, _ in nested_tail)
    apart = _answers(world, [(1, [9]), (1, [10])], [], [[1, 2, 3], [1, 5, 3]], 31)
    assert all(not a and len(hard) >= 2 for a, hard in apart)
    apart_tail = _answers(world, [(1, [9]), (1, [10])], [1], [[1, 2, 3], [1, 5, 3]], 32)
    assert all(not a for a, _ in apart_tail) and any(hard for _, hard in apart_tail)


def test_optional_outputs(be):
    """hard = NULL, counts = NULL: the answers are the same and nothing else is written; counts without hard: zeros"""
    world = _seven_world(be)
    rng = np.random.RandomState(3)
    for qt in ('3-inter', '3-chain_inter'):
        branches, tail = SEVEN[qt]
        prog, target = world.programme(branches, tail)
        n_out = int(world.mode_rows[target])
        anchors = np.stack([rng.randint(0, world.mode_rows[m], size=5) for m, _ in branches])
        full = _call(world, prog, anchors, n_out, rng, 0)
        for flags in (0, _capi.KG_GLOBAL_BITS):
            bare = _call(world, prog, anchors, n_out, rng, flags, hard=False, counts=False)
            np.testing.assert_array_equal(bare[0], full[0])
            some = _call(world, prog, anchors, n_out, rng, flags, hard=False)
            np.testing.assert_array_equal(some[0], full[0])
            np.testing.assert_array_equal(some[2], np.stack([full[2][0], np.zeros(5, dtype=np.int64)]))


def test_out_of_range_anchor(be):
    """Anchor rows n and -1: MPQE_FLAG_BAD_INDEX, those queries' sets are empty (every word written), the others exact"""
    world = _seven_world(be)
    branches, tail = SEVEN['3-inter']
    anchors = np.array([[1, 2, 33, 4, 5], [7, 8, 9, 10, -1], [3, 3, 3, 3, 3]])
    want = _answers(world, branches, tail, anchors, 40, want_flags=BAD_INDEX)
    assert want[2] == (set(), set()) and want[4] == (set(), set())
    branches, tail = SEVEN['3-chain_inter']
    _answers(world, branches, tail, np.array([[65, 2, 3], [1, 2, 3]]), 41, want_flags=BAD_INDEX)
    _answers(world, branches, tail, np.array([[64, 2, 3], [1, 2, 32]]), 42)          # the last rows: in range


# ---------------------------------------------------------------------------------------------- a corrupt index
CORRUPT_ROWS = [1, 33, 65]
A0, B0, X = 10, 20, 64          # query 0's anchors (branch 0, branch 1) and the one row of mode 2 that only query 0 reaches


def _corrupt_relations():
    """Modes of 1, 33 and 65 rows. 0 and 3: mode 1 -> mode 2, the first hops; row X is in the lists of A0 (relation 0) and B0
    (relation 3) only. 1, 2 and 4: mode 2 -> modes 1, 0 and 2, the hops a frontier scan walks; X's lists hold four entries."""
    rng = np.random.RandomState(23)
    first = lambda: {r: rng.randint(0, X, size=3).tolist() for r in range(33)}          # noqa: E731
    scan = lambda n: {r: rng.randint(0, n, size=rng.randint(1, 5)).tolist() for r in range(65)}     # noqa: E731
    rels = [(1, 2, first()), (2, 1, scan(33)), (2, 0, scan(1)), (1, 2, first()), (2, 2, scan(65))]
    rels[0][2][A0] = [5, X, 9]
    rels[3][2][B0] = [X, 3]
    rels[1][2][X] = [32, 0, 7, 32]
    rels[2][2][X] = [0, 0, 0, 0]
    rels[4][2][X] = [X, 1, 0, 33]
    return rels


@pytest.mark.parametrize('qt', ['2-chain', '3-chain_inter'])
@pytest.mark.parametrize('fault', ['offset', 'row to 1 row', 'row to 33 rows', 'row to 65 rows'])
def test_corrupt_csr_is_flagged_and_the_rest_of_the_set_kept(be, fault, qt):
    """The index lies in one place, which only query 0 of 4 meets. 'offset': offsets[A0 + 1] of the first hop's relation is
    past `edges` -- the anchor's list is walked clamped to [offsets[A0], edges). 'row': entry 1 of row X's list in the
    relation the frontier scan walks is the destination mode's row count (the first row outside it; its bit would lie inside
    the mode's last word for 1 and 33 rows) -- the entry is skipped, the list's other three are followed. Either way
    MPQE_FLAG_BAD_INDEX is set, query 0 gets what the oracle gets on the clamped / shortened list, and the other three
    queries get the words of the clean index. Both homes of the bitmaps; guards checked by _call."""
    rels = _corrupt_relations()
    clean = World(be, CORRUPT_ROWS, rels)
    bad = World(be, CORRUPT_ROWS, rels)
    walked = [(s, d, dict(lists)) for s, d, lists in rels]             # what the kernel is to make of the corrupt index
    if fault == 'offset':
        scan = 1
        edges = int(bad.edges[0])
        flat = [x for r in range(33) for x in rels[0][2][r]]
        lo = sum(len(rels[0][2][r]) for r in range(A0))
        bad.keep[0][A0 + 1] = edges + 7
        walked[0][2][A0] = flat[lo:edges]
        walked[0][2][A0 + 1] = []                                       # (its lower end is past `edges`; nobody's anchor)
        assert len(flat) == edges and set(rels[0][2][A0]) < set(walked[0][2][A0])
    else:
        scan = {'row to 1 row': 2, 'row to 33 rows': 1, 'row to 65 rows': 4}[fault]
        n_dst = CORRUPT_ROWS[rels[scan][1]]
        at = sum(len(rels[scan][2][r]) for r in range(X)) + 1
        bad.keep[2 * scan + 1][at] = n_dst
        walked[scan][2][X] = rels[scan][2][X][:1] + rels[scan][2][X][2:]
    bad.relations = walked
    branches, tail = ([(1, [0, scan])], []) if qt == '2-chain' else ([(1, [0]), (1, [3])], [scan])
    anchors = np.array([[A0, 1, 2, 3], [B0, 4, 5, 6]][:len(branches)])
    prog, target = clean.programme(branches, tail)
    n_out = CORRUPT_ROWS[target]
    want = bad.oracle(branches, tail, anchors)
    assert want[1:] == clean.oracle(branches, tail, anchors)[1:]
    if fault != 'offset':
        assert set(walked[scan][2][X]) <= want[0][0] and n_dst not in want[0][0] | want[0][1]
    want_a = np.stack([_bitmap(w[0], n_out) for w in want])
    want_h = np.stack([_bitmap(w[1], n_out) for w in want])
    want_c = np.array([[len(w[0]) for w in want], [len(w[1]) for w in want]], dtype=np.int64)
    rng = np.random.RandomState(60)
    for flags in (0, _capi.KG_GLOBAL_BITS):
        what = 'bitmaps in %s' % ('the workspace' if flags else 'LDS')
        got_a, got_h, got_c, err = _call(bad, prog, anchors, n_out, rng, flags)
        ref_a, ref_h, ref_c, ref_err = _call(clean, prog, anchors, n_out, rng, flags)
        assert err == BAD_INDEX and ref_err == 0, what
        np.testing.assert_array_equal(got_a, want_a, err_msg='answers, ' + what)
        np.testing.assert_array_equal(got_h, want_h, err_msg='hard, ' + what)
        np.testing.assert_array_equal(got_c, want_c, err_msg='counts, ' + what)
        np.testing.assert_array_equal(got_a[1:], ref_a[1:], err_msg='the other queries, ' + what)
        np.testing.assert_array_equal(got_h[1:], ref_h[1:], err_msg='the other queries (hard), ' + what)
        np.testing.assert_array_equal(got_c[:, 1:], ref_c[:, 1:], err_msg='the other queries (counts), ' + what)


def test_same_call_twice_gives_the_same_bits(be):
    world = _seven_world(be)
    branches, tail = SEVEN['3-chain_inter']
    prog, target = world.programme(branches, tail)
    rng = np.random.RandomState(50)
    anchors = np.stack([rng.randint(0, world.mode_rows[m], size=17) for m, _ in branches])
    one = _call(world, prog, anchors, int(world.mode_rows[target]), rng, 0)
    two = _call(world, prog, anchors, int(world.mode_rows[target]), rng, 0)
    assert all(np.array_equal(a, b) for a, b in zip(one[:3], two[:3])) and one[3] == two[3] == 0


# ---------------------------------------------------------------------------------------------- mpqe_kg_rows
def _rows_call(be, rng, bits, n, valid, select, lengths, slack=0):
    """-> (offsets, the rows written [total], error word); rows_out between guards, `slack` unused slots behind the lists"""
    Q = bits.shape[0]
    off = np.zeros(Q + 1, dtype=np.int64)
    off[1:] = np.cumsum(lengths)
    total = int(off[-1])
    d_bits = _at(be, bits.view(np.int32), 4)
    d_valid = None if valid is None else _at(be, valid.view(np.int32), 4)
    d_off = _at(be, off, 8)
    buf, view, before = _fenced(be, rng, total + slack + 1, item=8)
    err = be.zeros((1,), np.int32)
    be.check(be.lib.mpqe_kg_rows(be.ptr(d_bits), Q, n, be.ptr(d_valid), select, be.ptr(d_off), be.ptr(view), total + slack,
                                 be.ptr(err), be.stream), 'mpqe_kg_rows')
    _guards_kept(be, buf, before, total + slack + 1, 'rows_out')
    out = be.get(view)
    np.testing.assert_array_equal(out[total:], before[GUARD + total:GUARD + total + slack + 1], err_msg='slots behind the lists')
    np.testing.assert_array_equal(be.get(d_bits).view(np.uint32), bits)           # (read only)
    return off, out[:total].copy(), int(be.get(err)[0])


@pytest.mark.parametrize('n', [1, 33, 2049, 8200])
def test_rows_of_bitmaps(be, n):
    """Bitmaps -> ascending row lists, for the three selections; n = 8 200 is 257 words: two rounds of the workgroup. One
    query's set is empty, one holds all n rows; the input's bits at or above n are set (they name no row); `valid` has
    holes, which never come out of the complement and always out of WITH_HOLES."""
    rng = np.random.RandomState(n)
    W = _words(n)
    Q = 5
    member = rng.rand(Q, n) < 0.3
    member[1] = False
    member[2] = True
    is_valid = rng.rand(n) < 0.8
    is_valid[n - 1] = n > 1
    pad = np.ones((Q, W * 32 - n), dtype=bool)                         # stray bits behind row n - 1
    bits = np.packbits(np.concatenate([member, pad], axis=1), axis=1, bitorder='little').view(np.uint32).reshape(Q, W)
    valid = np.packbits(np.concatenate([is_valid, pad[0]]), bitorder='little').view(np.uint32)
    for select, chosen, vmap in ((_capi.KG_ROWS_SET, member, valid), (_capi.KG_ROWS_SET, member, None),
                                 (_capi.KG_ROWS_COMPLEMENT, is_valid[None, :] & ~member, valid),
                                 (_capi.KG_ROWS_COMPLEMENT, ~member, None),
                                 (_capi.KG_ROWS_WITH_HOLES, member | ~is_valid[None, :], valid)):
        lengths = chosen.sum(axis=1)
        off, rows, err = _rows_call(be, rng, bits, n, vmap, select, lengths, slack=2)
        assert err == 0 and off[Q] == chosen.sum() == rows.shape[0]
        for q in range(Q):
            np.testing.assert_array_equal(rows[off[q]:off[q + 1]], np.nonzero(chosen[q])[0],
                                          err_msg='select %d, query %d' % (select, q))
    assert not member[1].any() and member[2].all()


def test_rows_that_do_not_fit_are_flagged_not_written(be):
    """offsets that promise one slot too few for query 1, and one too many for query 2: MPQE_FLAG_BAD_INDEX; nothing lands
    outside a query's own segment (query 1's last row is dropped, query 2's spare slot keeps its bits)"""
    rng = np.random.RandomState(2)
    n = 70
    member = rng.rand(3, n) < 0.5
    bits = np.packbits(np.concatenate([member, np.zeros((3, 96 - n), dtype=bool)], axis=1), axis=1,
                       bitorder='little').view(np.uint32).reshape(3, 3)
    true = member.sum(axis=1)
    lengths = true + np.array([0, -1, 1])
    off, rows, err = _rows_call(be, rng, bits, n, None, _capi.KG_ROWS_SET, lengths)
    assert err == BAD_INDEX
    np.testing.assert_array_equal(rows[off[0]:off[1]], np.nonzero(member[0])[0])
    np.testing.assert_array_equal(rows[off[1]:off[2]], np.nonzero(member[1])[0][:-1])
    np.testing.assert_array_equal(rows[off[2]:off[3] - 1], np.nonzero(member[2])[0])
