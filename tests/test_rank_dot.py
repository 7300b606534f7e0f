"""mpqe_rank_entities_scored with score_kind 1: every row of a table ranked against Q query embeddings by the plain dot
product q[i] . table[r] -- the score the diagonal path decoder gives a chain query. Host emulator and gfx950 library, the
shapes, helpers and tolerance of tests/test_rank.py.

Truth is float64 numpy: s64 = q @ table.T. The tolerance tol(s) = 2e-6 + 1e-5 |s| of tests/test_rank.py is kept; it
means something for a dot product only while eps32 * |q[i]| * |table[r]| stays well below it, so the operands are what
answer() hands the kernel: unit-length queries (normalised anchors) and candidate rows of length 2 .. 8 (a normalised row
scaled by a vector of entries up to 6 / sqrt(D) a few times over). Scores then reach well above 1 in size, with both signs.
test_tolerance_covers_plain_fp32 confirms on the CPU that plain fp32 numpy stays inside the tolerance at every shape used.
Integers are compared exactly."""
import numpy as np
import pytest

from tests.test_rank import (EPS, ERR_INVALID_ARG, MAX_K, SHAPES, be, check_rank, check_topk, csr,  # noqa: F401
                             random_excl, run as run_cosine, tol)

DOT, COSINE = 1, 0


def truth(q, table):
    return q.astype(np.float64) @ table.astype(np.float64).T


def make(seed, Q, N, D, lo=2.0, hi=8.0):
    """Unit queries, rows of length lo .. hi; query i leans towards (even i) or away from (odd i) one row, so that scores
    well above 1 in size exist with both signs at every D."""
    rng = np.random.RandomState(seed)
    unit = lambda a: a / np.linalg.norm(a, axis=1, keepdims=True)      # noqa: E731
    t = unit(rng.randn(N, D))
    sign = np.where(np.arange(Q) % 2 == 0, 1.0, -1.0)[:, None]
    q = unit(0.8 * sign * t[rng.randint(0, N, size=Q)] + 0.6 * unit(rng.randn(Q, D))).astype(np.float32)
    t = (t * (lo + (hi - lo) * rng.rand(N, 1))).astype(np.float32)
    target = rng.randint(0, N, size=Q).astype(np.int64)
    return rng, q, t, target


def run(be, q, table, target=None, excl=None, k=0, kind=DOT, status=0, eps=EPS):
    Q, D = q.shape
    N = table.shape[0]
    dq, dt = be.put(q), be.put(table)
    dtarget = None if target is None else be.put(np.asarray(target, dtype=np.int64))
    off = rows = None
    E = 0
    if excl is not None:
        o, r = csr(excl, Q)
        E = int(r.shape[0])
        off, rows = be.put(o), be.put(r if E else np.zeros(1, dtype=np.int64))
    topr = be.empty((Q, max(k, 1)), np.int64) if k > 0 else None
    tops = be.empty((Q, max(k, 1)), np.float32) if k > 0 else None
    rank = be.empty((Q,), np.int64) if target is not None else None
    tsc = be.empty((Q,), np.float32) if target is not None else None
    need = be.lib.mpqe_rank_workspace_bytes(Q, N, D, k)
    ws = be.nbytes(need)
    err = be.zeros((1,), np.int32)
    st = be.lib.mpqe_rank_entities_scored(be.ptr(dq), Q, be.ptr(dt), N, D, eps, kind, be.ptr(dtarget), be.ptr(off),
                                          be.ptr(rows), E, k, be.ptr(topr), be.ptr(tops), be.ptr(rank), be.ptr(tsc),
                                          be.ptr(ws), need, be.ptr(err), be.stream)
    assert st == status, 'status %d, expected %d' % (st, status)
    get = lambda a: None if a is None else be.get(a)       # noqa: E731
    return {'rows': get(topr), 'scores': get(tops), 'rank': get(rank), 'tscore': get(tsc), 'err': int(be.get(err)[0])}


def test_tolerance_covers_plain_fp32():
    """No kernel involved: the dot product in plain fp32 numpy against float64, at every dim the tests use."""
    worst = 0.0
    for (Q, N, D, k) in SHAPES + [(64, 300, 7, 5)]:
        _, q, table, _ = make(11 + D, max(Q, 32), max(N, 200), D)
        s64 = truth(q, table)
        s32 = q @ table.T
        assert s32.dtype == np.float32
        worst = max(worst, float((np.abs(s32 - s64) / tol(s64)).max()))
        assert s64.max() > 2.0 and s64.min() < -2.0         # (|score| well above 1, both signs, in every shape)
    print('worst |fp32 - fp64| / tolerance: %.3g' % worst)
    assert worst <= 0.5


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'Q%d_N%d_D%d_k%d' % s)
def test_rank_and_topk_by_dot(be, shape):
    """(67, 700, 48, 10): eleven column tiles, one per strip (eleven strips: tests/test_operand_bounds.py and
    tests/test_rank_exact.py have the shapes with several tiles per strip); k up to 128."""
    Q, N, D, k = shape
    _, q, table, target = make(100 + Q, Q, N, D)
    s64 = truth(q, table)
    out = run(be, q, table, target, None, k)
    assert out['err'] == 0
    check_topk(out, s64, None, k)
    check_rank(out, s64, target, None)
    if Q > 1:
        assert (s64 < -1).any() and (s64 > 1).any()
    for i in range(Q):          # exact: the target sits at its rank
        r = int(out['rank'][i])
        if r <= k:
            assert out['rows'][i, r - 1] == target[i]
        else:
            assert target[i] not in out['rows'][i]


def test_the_norms_are_left_out(be):
    """Rows of very different lengths: the dot order differs from the cosine order, and the scores are the dots -- a kernel
    that still multiplied by 1 / |row| would return the cosine's."""
    Q, N, D, k = 5, 63, 10, 3
    _, q, table, target = make(105, Q, N, D)
    s64 = truth(q, table)
    cos = s64 / np.linalg.norm(table.astype(np.float64), axis=1)[None, :]
    assert (np.argmax(cos, axis=1) != np.argmax(s64, axis=1)).any()
    out = run(be, q, table, target, None, k)
    np.testing.assert_array_equal(out['rows'][:, 0], np.argmax(s64, axis=1))
    assert (np.abs(out['tscore'] - cos[np.arange(Q), target]) > 10 * tol(cos[np.arange(Q), target])).all()
    # eps is not read: a huge eps changes nothing, to the bit
    big = run(be, q, table, target, None, k, eps=1e30)
    for key in ('rows', 'rank'):
        np.testing.assert_array_equal(big[key], out[key])
    assert big['scores'].tobytes() == out['scores'].tobytes() and big['tscore'].tobytes() == out['tscore'].tobytes()


@pytest.mark.parametrize('shape', SHAPES[1:], ids=lambda s: 'Q%d_N%d_D%d_k%d' % s)
def test_exclusion_lists(be, shape):
    Q, N, D, k = shape
    rng, q, table, target = make(200 + Q, Q, N, D)
    excl = random_excl(rng, Q, N, target, 40)
    s64 = truth(q, table)
    out = run(be, q, table, target, excl, k)
    assert out['err'] == 0
    check_topk(out, s64, excl, k)
    check_rank(out, s64, target, excl)


def test_all_negative_scores(be):
    """Every score of every query below -1: nothing in the pipeline may take 0 (or -1) for "worse than any score"."""
    Q, N, D, k = 67, 300, 48, MAX_K
    rng, q, table, target = make(31, Q, N, D)
    q, table = np.abs(q), -np.abs(table) - np.float32(0.25)
    s64 = truth(q, table)
    assert s64.max() < -1.0
    excl = random_excl(rng, Q, N, target, 20)
    for e in (None, excl):
        out = run(be, q, table, target, e, k)
        assert out['err'] == 0
        check_topk(out, s64, e, k)
        check_rank(out, s64, target, e)
        assert (out['scores'][:, :k] < -1.0).all() and (out['rows'][:, :k] >= 0).all()


def test_ties_go_to_the_smaller_row(be):
    """Exact copies of a row give bit-equal dots: they lead in row order, and the rank counts the smaller copies only."""
    Q, N, D, k = 6, 200, 32, 20
    _, q, table, _ = make(3, Q, N, D)
    group = [150, 17, 64, 99, 3]
    for i in range(Q):
        q[i] = table[150] / np.float32(8.0) + np.float32(0.02) * q[i]
    table[150] *= np.float32(4.0)               # the longest row along every query: the best dot
    for r in group[1:]:
        table[r] = table[150]
    order = sorted(group)
    for t in group:
        target = np.full(Q, t, dtype=np.int64)
        out = run(be, q, table, target, None, k)
        for i in range(Q):
            assert out['rows'][i, :len(order)].tolist() == order
            assert len(set(out['scores'][i, :len(order)].view(np.int32).tolist())) == 1
            assert out['scores'][i, len(order)] < out['scores'][i, 0]
            assert out['rank'][i] == 1 + order.index(t)
            assert out['scores'][i, 0] > 1.0


def test_score_kind_0_is_the_old_entry_to_the_bit(be):
    from tests.test_rank import make as make_cosine
    Q, N, D, k = 97, 333, 64, 12
    rng, q, table, target = make_cosine(7, Q, N, D)
    excl = random_excl(rng, Q, N, target, 25)
    old = run_cosine(be, q, table, target, excl, k)
    new = run(be, q, table, target, excl, k, kind=COSINE)
    for key in ('rows', 'rank'):
        np.testing.assert_array_equal(old[key], new[key])
    for key in ('scores', 'tscore'):
        assert old[key].tobytes() == new[key].tobytes()
    dot = run(be, q, table, target, excl, k, kind=DOT)
    assert dot['scores'].tobytes() != old['scores'].tobytes()


def test_another_score_kind_is_refused(be):
    _, q, table, target = make(1, 4, 50, 16)
    for kind in (2, -1):
        out = run(be, q, table, target, None, 5, kind=kind, status=ERR_INVALID_ARG)
        assert np.isnan(out['scores']).all() and (out['rank'] == -7).all()      # (nothing was launched)
