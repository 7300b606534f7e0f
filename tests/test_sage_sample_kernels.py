"""mpqe_kg_sample_neighbours (csrc/sage.hip) through the C ABI, on the host emulator and (gpu) on the real library, against
tests/sage_oracle.py: bit parity with the stream restated with Python ints, properties that hold whatever the stream is, and
the uniform law of the sampled subsets (chi-square; fixed seeds, so deterministic; passes at p >= 1e-6 and prints p).

Operand hygiene is tests/test_kg_kernels.py's (its helpers are used): outputs sit between guard words that must keep their
bits and start as garbage, int64 operands start 8 bytes past a 16-byte boundary, int32 ones 4 bytes."""
import ctypes
import itertools

import numpy as np
import pytest

from mpqe_amd import _capi
from tests import kg_sample_oracle
from tests import sage_oracle as oracle
from tests import test_kg_kernels as K
from tests import test_kg_sample_kernels as S

be = K.be
BAD_INDEX = _capi.FLAG_BAD_INDEX
OK, INVALID = 0, -1
P_FLOOR = S.P_FLOOR
LENGTHS = (0, 1, 2, 3, 7, 10, 11, 33, 1000)
N_DST = 1200


def _relations():
    """mode 0 (12 rows) -> mode 1 (1 200 rows): row i has a list of LENGTHS[i] DISTINCT rows, unsorted (a position is then
    known by its value); rows 9 .. 11 have none. Relation 1: mode 0 -> mode 2, short random lists with repeats. Relation 2
    has no edge. Relation 3 leaves another mode."""
    rng = np.random.RandomState(5)
    first = {i: rng.permutation(N_DST)[:n].tolist() for i, n in enumerate(LENGTHS) if n}
    second = {i: rng.randint(0, 40, size=rng.randint(1, 6)).tolist() for i in range(12) if i % 3}
    return [(0, 1, first), (0, 2, second), (0, 1, {}), (1, 0, {3: [1, 2], 1199: [0]})]


ROWS = [12, N_DST, 40]


def _sample(world, use_rels, rows, keep_prob, max_keep, seed, rng):
    """one call -> (neigh [R, B, max_keep], counts [R, B], the error word)"""
    be = world.be
    R, B = len(use_rels), len(rows)
    d_rows = K._at(be, np.asarray(rows, dtype=np.int64), 8)
    use = np.asarray(use_rels, dtype=np.int32)
    n_buf, n_view, n_before = K._fenced(be, rng, R * B * max_keep, item=8)
    c_buf, c_view, c_before = K._fenced(be, rng, R * B)
    err = be.zeros((1,), np.int32)
    be.check(be.lib.mpqe_kg_sample_neighbours(world.offs, world.rows, world.edges, world.src.ctypes.data, world.dst.ctypes.data,
                                              len(world.relations), world.mode_rows.ctypes.data, len(world.mode_rows),
                                              use.ctypes.data, R, be.ptr(d_rows), B, keep_prob, max_keep, seed, be.ptr(n_view),
                                              be.ptr(c_view), be.ptr(err), be.stream), 'mpqe_kg_sample_neighbours')
    K._guards_kept(be, n_buf, n_before, R * B * max_keep, 'neigh')
    K._guards_kept(be, c_buf, c_before, R * B, 'counts')
    np.testing.assert_array_equal(be.get(d_rows), np.asarray(rows, dtype=np.int64))        # (read only)
    return be.get(n_view).reshape(R, B, max_keep).copy(), be.get(c_view).reshape(R, B).copy(), int(be.get(err)[0])


def _batch(rng, B):
    """every list length, null nodes and one node at several positions, as far as B allows"""
    rows = rng.randint(0, 12, size=B)
    rows[:min(B, 9)] = np.arange(9)[::-1][:min(B, 9)]           # the long list first
    if B > 20:
        rows[10], rows[15] = -1, -1
        rows[[11, 12, 19]] = 4                                  # the node of 7 neighbours three times
    return rows.astype(np.int64)


# ---------------------------------------------------------------------------------------------- 1. bit parity
@pytest.mark.parametrize('B', [1, 63, 64, 65])
def test_samples_equal_the_restated_stream(be, B):
    world = S.SampleWorld(be, ROWS, _relations())
    rng = np.random.RandomState(B)
    rows = _batch(rng, B)
    drawn = 0
    for use_rels in ([0], [1, 2, 0]):
        for keep_prob, max_keep in itertools.product((1.0, 0.5, 0.7, 0.05), (1, 2, 10, 32)):
            seed = 2 ** 63 + 77 if max_keep == 2 else 1000 * max_keep + int(100 * keep_prob)
            neigh, counts, err = _sample(world, use_rels, rows, keep_prob, max_keep, seed, rng)
            want_n, want_c = oracle.sample_neighbours(world.relations, use_rels, rows, keep_prob, max_keep, seed)
            what = 'relations %s, keep_prob %s, max_keep %d' % (use_rels, keep_prob, max_keep)
            np.testing.assert_array_equal(counts, want_c, err_msg=what)
            np.testing.assert_array_equal(neigh, want_n, err_msg=what)
            assert err == 0, what
            drawn += int((counts > 0).sum())
    assert drawn > 0


# ---------------------------------------------------------------------------------------------- 2. whatever the stream
def test_properties_that_hold_for_any_stream(be):
    """count = the reference's expression; the entries are DISTINCT positions of the node's own list (relation 0's lists
    hold distinct rows); unused slots are -1; a node at two positions draws twice (the draws differ somewhere)."""
    world = S.SampleWorld(be, ROWS, _relations())
    rng = np.random.RandomState(3)
    rows = np.array([8] * 40 + [-1, 0, 9] + list(range(9)) * 3, dtype=np.int64)
    lists = world.relations[0][2]
    for keep_prob, max_keep in ((0.5, 10), (0.7, 32), (0.05, 32), (1.0, 2)):
        neigh, counts, err = _sample(world, [0, 2], rows, keep_prob, max_keep, 99, rng)
        assert err == 0
        assert (counts[1] == 0).all() and (neigh[1] == -1).all()                   # the relation without edges
        for b, x in enumerate(rows):
            lst = lists.get(int(x), []) if x >= 0 else []
            k = min(int(np.ceil(len(lst) * keep_prob)), max_keep) if lst else 0
            assert counts[0, b] == k, (keep_prob, max_keep, b)
            got = neigh[0, b, :k].tolist()
            assert len(set(got)) == k and set(got) <= set(lst)
            assert (neigh[0, b, k:] == -1).all()
            if k == len(lst):
                assert got == lst                                                 # the list in CSR order, no draw
        if 0 < counts[0, 0] < 1000:
            assert len(set(tuple(neigh[0, b]) for b in range(40))) > 1


# ---------------------------------------------------------------------------------------------- 3. uniformity
def test_sampled_subsets_are_uniform(be):
    """One node with 7 neighbours, k = ceil(7 * 0.4) = 3, 20 000 positions of that node in four calls: the counts of the 35
    subsets against the exact uniform law, by the statistic of tests/kg_sample_oracle.py."""
    world = S.SampleWorld(be, ROWS, _relations())
    rng = np.random.RandomState(4)
    lst = world.relations[0][2][4]
    assert len(lst) == 7
    observed, total = {}, 0
    for seed in (11, 12, 13, 14):
        neigh, counts, err = _sample(world, [0], np.full(5000, 4, dtype=np.int64), 0.4, 10, seed, rng)
        assert err == 0 and (counts == 3).all()
        for picks in neigh[0, :, :3].tolist():
            key = frozenset(picks)
            observed[key] = observed.get(key, 0) + 1
        total += 5000
    dist = {frozenset(c): 1.0 / 35 for c in itertools.combinations(lst, 3)}
    stat, dof, p = kg_sample_oracle.chi_square(observed, dist, total)
    print('subsets (%s): chi2 %.1f, dof %d, p %.3g' % (be.name, stat, dof, p))
    assert dof == 34 and p >= P_FLOOR


# ---------------------------------------------------------------------------------------------- 4. corrupt input
def test_bad_rows_and_offsets_are_flagged_and_not_followed(be):
    """A source row at its mode's row count, a list whose end lies beyond the relation's edges, and a neighbour outside its
    mode: MPQE_FLAG_BAD_INDEX; the first two get count 0 and -1 slots, the third a -1 in its slot; the other positions are
    exact, and nothing lands outside the outputs (_sample checks the guards)."""
    world = S.SampleWorld(be, ROWS, _relations())
    rng = np.random.RandomState(6)
    rows = np.array([3, 12, 5, 7, 2], dtype=np.int64)
    want_n, want_c = oracle.sample_neighbours(world.relations, [0], rows, 1.0, 32, 5)
    neigh, counts, err = _sample(world, [0], rows, 1.0, 32, 5, rng)
    assert err == BAD_INDEX and counts[0, 1] == 0 and (neigh[0, 1] == -1).all()
    keep = [0, 2, 3, 4]
    np.testing.assert_array_equal(neigh[0, keep], want_n[0, keep])
    off = world.d_offsets(0)
    off[6] = int(world.edges[0]) + 3                    # row 5's list: [lo, edges + 3)
    world.d_rows(0)[int(np.cumsum(LENGTHS)[1])] = N_DST             # row 2's first neighbour: outside mode 1
    neigh, counts, err = _sample(world, [0], np.array([3, 5, 2, 7], dtype=np.int64), 1.0, 32, 5, rng)
    assert err == BAD_INDEX
    assert counts[0].tolist() == [3, 0, 2, 32] and (neigh[0, 1] == -1).all()
    assert neigh[0, 2, 0] == -1 and neigh[0, 2, 1] == want_n[0, 4, 1]
    np.testing.assert_array_equal(neigh[0, [0, 3]], want_n[0, [0, 3]])


# ---------------------------------------------------------------------------------------------- 5. refused before launch
@pytest.mark.parametrize('which', ['emu', 'product'])
def test_refused_before_any_launch(which):
    """Device pointers are made-up addresses: a call that launched anything with them would fault."""
    lib = S._libs()[which]()
    fake = 0x10000
    R = 3
    ptrs = (ctypes.c_void_p * R)(fake, fake, fake)
    edges = (ctypes.c_int64 * R)(7, 0, 4)
    src, dst = np.array([0, 0, 1], dtype=np.int32), np.array([1, 0, 0], dtype=np.int32)
    mode_rows = np.array([40, 100], dtype=np.int64)

    def call(offs=ptrs, use=(0, 1), rows=fake, B=5, keep_prob=0.5, max_keep=10, neigh=fake, counts=fake, M=2, nrel=R):
        u = np.asarray(use, dtype=np.int32)
        return lib.mpqe_kg_sample_neighbours(offs, ptrs, edges, src.ctypes.data, dst.ctypes.data, nrel, mode_rows.ctypes.data, M,
                                             u.ctypes.data if u.size else None, u.size, rows, B, keep_prob, max_keep, 1, neigh,
                                             counts, None, None)
    assert call(max_keep=0) == INVALID and call(max_keep=_capi.SAGE_MAX_KEEP + 1) == INVALID
    assert call(keep_prob=0.0) == INVALID and call(keep_prob=1.5) == INVALID and call(keep_prob=float('nan')) == INVALID
    assert call(keep_prob=-0.5) == INVALID
    assert call(use=()) == INVALID and call(use=[0] * 65) == INVALID and call(use=(0, 3)) == INVALID and call(use=(-1,)) == INVALID
    assert call(use=(0, 2)) == INVALID                                      # two source modes
    assert call(offs=(ctypes.c_void_p * R)(fake, None, fake)) == INVALID and call(offs=None) == INVALID
    assert call(B=-1) == INVALID and call(rows=None) == INVALID and call(neigh=None) == INVALID and call(counts=None) == INVALID
    assert call(M=0) == INVALID and call(M=17) == INVALID and call(nrel=0) == INVALID
    assert call(B=0) == OK and call(B=0, rows=None, neigh=None, counts=None) == OK      # nothing is launched
    assert _capi.SAGE_MAX_KEEP == 32


# ---------------------------------------------------------------------------------------------- 6. the index's method
def test_index_sample_neighbours_on_the_emulator():
    """KGIndex.rows_of + KGIndex.sample_neighbours on a CPU-resident index driven by the host emulator (lib=): ids to rows
    (a negative id stays the null node, a foreign id lands outside its mode), the relations in the caller's order, and the
    oracle's bits for the lists the index holds."""
    import torch
    from mpqe_amd import synthetic
    from mpqe_amd.data_utils import make_feature_modules
    from mpqe_amd.kg import KGIndex
    from tests.kernel_backend import EmuBackend
    schema = synthetic.make_schema(*synthetic.KG_SHAPES['tiny'], seed=5)
    adj = synthetic.make_adjacency(schema, degree=3, seed=5)
    _, node_maps = make_feature_modules(schema.ids, 8, schema.num_entities)
    graph = synthetic.SchemaGraph(schema, 8)
    graph.adj_lists = adj
    index = KGIndex.from_graph(graph, node_maps, 'cpu', lib=EmuBackend().lib)
    mode, other = schema.modes[0], schema.modes[1]
    ids = [int(x) for x in schema.ids[mode][:9]] + [-1, int(schema.ids[other][0]), int(schema.ids[mode][0])]
    rows = index.rows_of(mode, torch.tensor(ids))
    n = int(index.mode_rows[index.mode_index[mode]])
    assert rows.tolist() == node_maps[ids[:9]].tolist() + [-1, n, int(node_maps[ids[0]])]
    rels = [(mode, name, to) for to, name in schema.relations[mode]][::-1]          # the caller's order, not the index's
    relations = []
    for rel in index.rels:
        off, lst = index.offsets[index.rel_index[rel]].numpy(), index.rows[index.rel_index[rel]].numpy()
        relations.append((0, 0, {x: lst[off[x]:off[x + 1]].tolist() for x in range(off.shape[0] - 1)}))
    use = [index.rel_index[r] for r in rels]
    got_rels, neigh, counts = index.sample_neighbours(mode, rows[:10], keep_prob=0.5, max_keep=2, seed=2 ** 64 + 5, relations=rels)
    want_n, want_c = oracle.sample_neighbours(relations, use, rows[:10].tolist(), 0.5, 2, 5)
    assert got_rels == rels and counts.dtype == torch.int32 and tuple(neigh.shape) == (len(rels), 10, 2)
    np.testing.assert_array_equal(neigh.numpy(), want_n)
    np.testing.assert_array_equal(counts.numpy(), want_c)
    assert int(index.err.item()) == 0 and (want_c > 0).any()
    _, neigh, counts = index.sample_neighbours(mode, rows, keep_prob=1.0, max_keep=32)      # row n: flagged, nothing drawn
    assert int(index.err.item()) == BAD_INDEX and (counts[:, 10] == 0).all() and (neigh[:, 10] == -1).all()
    with pytest.raises(KeyError):
        index.sample_neighbours(mode, rows, relations=[(other, 'r0', mode)])
