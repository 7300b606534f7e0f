"""mpqe_rank_entities: every row of a table ranked against Q query embeddings, rank of a target and fused top-k.

Runs on the host fiber emulator (`emu`, no GPU needed) and on the gfx950 library (`hip`, marked gpu).

Truth is float64 numpy: s64[i, r] = cos(q[i], table[r] / |table[r]|). Tolerance tol(s) = 2e-6 + 1e-5 |s|, the one
tests/test_kernels.py applies to mpqe_cosine_fwd's scores; test_tolerance_covers_plain_fp32 confirms on the CPU that a
plain fp32 numpy restatement of the score stays inside it at every dim tested here (worst deviation from float64 seen
there: 2.2e-7, at most 5 % of the tolerance, dims 7 to 256), so it is used as it stands. Integers are compared
exactly: the kernel's rank, top-k and exclusions must agree with each other to the bit.
"""
import numpy as np
import pytest

from mpqe_amd._capi import FLAG_BAD_INDEX

MAX_K = 128
EPS = 1e-8
ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -2, -3


@pytest.fixture(scope='module', params=['emu', pytest.param('hip', marks=pytest.mark.gpu)])
def be(request):
    from tests import kernel_backend
    if request.param == 'emu':
        return kernel_backend.EmuBackend()
    return kernel_backend.HipBackend()


def tol(s):
    return 2e-6 + 1e-5 * np.abs(s)


def close(a, b, what=''):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    bad = np.abs(a - b) > tol(b)
    assert not bad.any(), '%s: worst |diff| %.3g' % (what, np.abs(a - b).max())


def truth(q, table):
    q64, t64 = q.astype(np.float64), table.astype(np.float64)
    tn = t64 / np.linalg.norm(t64, axis=1, keepdims=True)
    nq = np.maximum(np.linalg.norm(q64, axis=1), EPS)
    nt = np.maximum(np.linalg.norm(tn, axis=1), EPS)
    return (q64 @ tn.T) / (nq[:, None] * nt[None, :])


def csr(excl, Q):
    off = np.zeros(Q + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(e) for e in excl])
    rows = np.array([r for e in excl for r in e], dtype=np.int64)
    return off, rows


def run(be, q, table, target=None, excl=None, k=0, want_rank=True, status=0, ws_bytes=None):
    """One call. excl: None or a list of (sorted) row lists. Returns a dict of numpy outputs plus the err word."""
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
    rank = be.empty((Q,), np.int64) if (target is not None and want_rank) else None
    tsc = be.empty((Q,), np.float32) if (target is not None and want_rank) else None
    need = be.lib.mpqe_rank_workspace_bytes(Q, N, D, k)
    ws = be.nbytes(need)
    err = be.zeros((1,), np.int32)
    st = be.lib.mpqe_rank_entities(be.ptr(dq), Q, be.ptr(dt), N, D, EPS, be.ptr(dtarget), be.ptr(off), be.ptr(rows), E, k,
                                   be.ptr(topr), be.ptr(tops), be.ptr(rank), be.ptr(tsc), be.ptr(ws),
                                   need if ws_bytes is None else ws_bytes, be.ptr(err), be.stream)
    assert st == status, 'status %d, expected %d' % (st, status)
    get = lambda a: None if a is None else be.get(a)
    return {'rows': get(topr), 'scores': get(tops), 'rank': get(rank), 'tscore': get(tsc), 'err': int(be.get(err)[0])}


def check_topk(out, s64, excl, k):
    Q, N = s64.shape
    for i in range(Q):
        banned = set(excl[i]) if excl is not None else set()
        eligible = [r for r in range(N) if r not in banned]
        n = min(k, len(eligible))
        rows, sc = out['rows'][i], out['scores'][i]
        got = rows[:n]
        assert len(set(got.tolist())) == n and (got >= 0).all() and (got < N).all(), 'distinct, in range (query %d)' % i
        assert not (set(got.tolist()) & banned), 'an excluded row was returned (query %d)' % i
        assert (rows[n:] == -1).all() and np.isneginf(sc[n:]).all(), 'tail must be -1 / -inf (query %d)' % i
        if n == 0:
            continue
        close(sc[:n], s64[i, got], 'top-k scores of query %d' % i)
        for j in range(1, n):
            assert sc[j - 1] > sc[j] or (sc[j - 1] == sc[j] and got[j - 1] < got[j]), 'total order (query %d)' % i
        rest = np.array([r for r in eligible if r not in set(got.tolist())], dtype=np.int64)
        if rest.size:
            kth = s64[i, got[n - 1]]
            assert (s64[i, rest] <= kth + 2 * tol(kth)).all(), 'a better row was left out (query %d)' % i


def check_rank(out, s64, target, excl):
    Q, N = s64.shape
    close(out['tscore'], s64[np.arange(Q), target], 'target scores')
    for i in range(Q):
        t = int(target[i])
        banned = set(excl[i]) if excl is not None else set()
        others = np.array([r for r in range(N) if r != t and r not in banned], dtype=np.int64)
        st = s64[i, t]
        so = s64[i, others] if others.size else np.zeros(0)
        lo = 1 + int((so > st + 2 * tol(st)).sum())
        hi = 1 + int((so >= st - 2 * tol(st)).sum())
        assert lo <= out['rank'][i] <= hi, 'rank %d outside [%d, %d] (query %d)' % (out['rank'][i], lo, hi, i)


def make(seed, Q, N, D, scale=1.0):
    rng = np.random.RandomState(seed)
    q = rng.randn(Q, D).astype(np.float32)
    table = (rng.randn(N, D) * scale * (0.5 + rng.rand(N, 1))).astype(np.float32)
    target = rng.randint(0, N, size=Q).astype(np.int64)
    return rng, q, table, target


def random_excl(rng, Q, N, target, most):
    excl = []
    for i in range(Q):
        n = rng.randint(0, min(most, N) + 1)
        rows = set(rng.choice(N, size=n, replace=False).tolist())
        if i % 2 == 0:
            rows.add(int(target[i]))         # filtered evaluation lists the target among the known answers
        excl.append(sorted(rows))
    return excl


SHAPES = [(1, 1, 16, 1), (5, 63, 10, 3), (67, 700, 48, 10), (130, 257, 128, 32), (64, 128, 256, MAX_K)]


def test_tolerance_covers_plain_fp32():
    """No kernel involved: the score restated in plain fp32 numpy against float64, at every dim the tests use."""
    for (Q, N, D, k) in SHAPES + [(64, 300, 7, 5)]:
        _, q, table, _ = make(11 + D, max(Q, 32), max(N, 200), D)
        s64 = truth(q, table)
        tn = table / np.sqrt((table * table).sum(axis=1, dtype=np.float32))[:, None]
        s32 = (q @ tn.T) / (np.maximum(np.sqrt((q * q).sum(axis=1, dtype=np.float32)), np.float32(EPS))[:, None]
                            * np.maximum(np.sqrt((tn * tn).sum(axis=1, dtype=np.float32)), np.float32(EPS))[None, :])
        assert s32.dtype == np.float32
        assert (np.abs(s32 - s64) <= tol(s64)).all(), 'dim %d: %.3g' % (D, np.abs(s32 - s64).max())


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'Q%d_N%d_D%d_k%d' % s)
def test_rank_and_topk_plain(be, shape):
    Q, N, D, k = shape
    _, q, table, target = make(100 + Q, Q, N, D)
    s64 = truth(q, table)
    out = run(be, q, table, target, None, k)
    assert out['err'] == 0
    check_topk(out, s64, None, k)
    check_rank(out, s64, target, None)
    for i in range(Q):          # exact: the target sits at its rank
        r = int(out['rank'][i])
        if r <= k:
            assert out['rows'][i, r - 1] == target[i], 'query %d: rank %d, top-k %s' % (i, r, out['rows'][i][:r + 1])
        else:
            assert target[i] not in out['rows'][i]


@pytest.mark.parametrize('shape', SHAPES[1:], ids=lambda s: 'Q%d_N%d_D%d_k%d' % s)
def test_rank_and_topk_with_exclusions(be, shape):
    Q, N, D, k = shape
    rng, q, table, target = make(200 + Q, Q, N, D)
    excl = random_excl(rng, Q, N, target, 40)
    s64 = truth(q, table)
    out = run(be, q, table, target, excl, k)
    assert out['err'] == 0
    check_topk(out, s64, excl, k)
    check_rank(out, s64, target, excl)
    # exact: with the target taken off its own list, its position in the top-k is its rank
    freed = [[r for r in e if r != target[i]] for i, e in enumerate(excl)]
    out2 = run(be, q, table, target, freed, k)
    np.testing.assert_array_equal(out2['rank'], out['rank'])
    for i in range(Q):
        r = int(out2['rank'][i])
        if r <= k:
            assert out2['rows'][i, r - 1] == target[i]
        else:
            assert target[i] not in out2['rows'][i]


def test_same_call_twice_and_split_calls_are_bit_identical(be):
    Q, N, D, k = 97, 333, 64, 12
    rng, q, table, target = make(7, Q, N, D)
    excl = random_excl(rng, Q, N, target, 25)
    a = run(be, q, table, target, excl, k)
    b = run(be, q, table, target, excl, k)
    for key in ('rows', 'rank'):
        np.testing.assert_array_equal(a[key], b[key])
    for key in ('scores', 'tscore'):
        np.testing.assert_array_equal(a[key].view(np.int32), b[key].view(np.int32))
    cut = 33
    lo = run(be, q[:cut], table, target[:cut], excl[:cut], k)
    hi = run(be, q[cut:], table, target[cut:], excl[cut:], k)
    for key in ('rows', 'rank'):
        np.testing.assert_array_equal(a[key], np.concatenate([lo[key], hi[key]]))
    for key in ('scores', 'tscore'):
        np.testing.assert_array_equal(a[key].view(np.int32), np.concatenate([lo[key], hi[key]]).view(np.int32))


def test_constructed_exact_ties(be):
    """Duplicates and power-of-two multiples of a row normalise to the same direction up to the rounding of 1/|row|;
    the copies here are exact duplicates and x2 / x0.5 / x4 copies, whose products, sums and norms scale exactly."""
    Q, N, D, k = 6, 200, 32, 20
    rng, q, table, _ = make(3, Q, N, D)
    group = [150, 17, 64, 99, 3]                   # all copies of row 150's direction
    for r, f in zip(group[1:], (1.0, 2.0, 0.5, 4.0)):
        table[r] = table[150] * np.float32(f)
    for i in range(Q):                             # the group is every query's best direction
        q[i] = table[150] * np.float32(2.0 ** -i) + np.float32(0.05) * q[i]
    order = sorted(group)
    for t in group:
        target = np.full(Q, t, dtype=np.int64)
        out = run(be, q, table, target, None, k)
        for i in range(Q):
            # the tied rows lead, the smaller row first, with bit-equal scores; the rank counts only the smaller ones
            assert out['rows'][i, :len(order)].tolist() == order, 'query %d: %s' % (i, out['rows'][i])
            assert len(set(out['scores'][i, :len(order)].view(np.int32).tolist())) == 1, 'tied rows have bit-equal scores'
            assert out['scores'][i, len(order)] < out['scores'][i, 0]
            assert out['rank'][i] == 1 + order.index(t)
        # excluding a smaller tied row moves the target up by exactly one
        if order.index(t) > 0:
            out2 = run(be, q, table, target, [[order[0]]] * Q, k)
            assert (out2['rank'] == order.index(t)).all()
            assert all(out2['rows'][i, :len(order) - 1].tolist() == order[1:] for i in range(Q))


def test_k_above_rows_and_modes_of_the_call(be):
    Q, N, D = 9, 20, 24
    rng, q, table, target = make(5, Q, N, D)
    s64 = truth(q, table)
    out = run(be, q, table, target, None, 30)                  # k > N
    check_topk(out, s64, None, 30)
    assert (out['rows'][:, N:] == -1).all()
    only_rank = run(be, q, table, target, None, 0)             # k = 0: ranks only
    np.testing.assert_array_equal(only_rank['rank'], out['rank'])
    only_topk = run(be, q, table, None, None, 7)               # no targets: top-k only
    np.testing.assert_array_equal(only_topk['rows'], out['rows'][:, :7])
    empty = run(be, q, table, target, [[] for _ in range(Q)], 7)       # an empty exclusion list
    np.testing.assert_array_equal(empty['rows'], out['rows'][:, :7])
    np.testing.assert_array_equal(empty['rank'], out['rank'])
    everything = [list(range(N)) for _ in range(Q)]            # a list that excludes every row
    none_left = run(be, q, table, target, everything, 7)
    assert (none_left['rows'] == -1).all() and np.isneginf(none_left['scores']).all()
    assert (none_left['rank'] == 1).all()
    mixed = [everything[0]] + [[] for _ in range(Q - 1)]
    out3 = run(be, q, table, target, mixed, 7)
    np.testing.assert_array_equal(out3['rows'][1:], out['rows'][1:, :7])
    assert (out3['rows'][0] == -1).all()


def test_repeated_rows_in_an_exclusion_list_count_once(be):
    Q, N, D, k = 4, 90, 16, 8
    rng, q, table, target = make(9, Q, N, D)
    excl = random_excl(rng, Q, N, target, 30)
    doubled = [sorted(e + e[::2]) for e in excl]
    a, b = run(be, q, table, target, excl, k), run(be, q, table, target, doubled, k)
    np.testing.assert_array_equal(a['rank'], b['rank'])
    np.testing.assert_array_equal(a['rows'], b['rows'])
    assert b['err'] == 0


def test_refusals(be):
    Q, N, D, k = 4, 50, 16, 5
    _, q, table, target = make(1, Q, N, D)
    lib = be.lib
    dq, dt, dtg = be.put(q), be.put(table), be.put(target)
    topr, tops = be.empty((Q, k), np.int64), be.empty((Q, k), np.float32)
    rank = be.empty((Q,), np.int64)
    need = lib.mpqe_rank_workspace_bytes(Q, N, D, k)
    ws = be.nbytes(need)
    err = be.zeros((1,), np.int32)

    def call(q_=dq, Q_=Q, N_=N, D_=D, k_=k, tg=dtg, need_=need, E_=0, rank_=rank):
        return lib.mpqe_rank_entities(be.ptr(q_), Q_, be.ptr(dt), N_, D_, EPS, be.ptr(tg), None, None, E_, k_,
                                      be.ptr(topr), be.ptr(tops), be.ptr(rank_), None, be.ptr(ws), need_, be.ptr(err),
                                      be.stream)
    assert call() == 0
    assert call(q_=None) == ERR_INVALID_ARG
    assert call(Q_=-1) == ERR_INVALID_ARG
    assert call(N_=-3) == ERR_INVALID_ARG
    assert call(N_=0) == ERR_INVALID_ARG
    assert call(D_=0) == ERR_INVALID_ARG
    assert call(k_=-1) == ERR_INVALID_ARG
    assert call(E_=3) == ERR_INVALID_ARG                   # entries announced, no lists
    assert call(tg=None) == ERR_INVALID_ARG                # a rank without targets
    assert call(k_=MAX_K + 1) == ERR_UNSUPPORTED
    assert lib.mpqe_rank_workspace_bytes(Q, N, D, MAX_K + 1) == 0
    assert call(need_=need - 1) == ERR_WORKSPACE
    assert call(Q_=0) == 0


def test_bad_rows_are_flagged_and_leave_the_rest_intact(be):
    Q, N, D, k = 70, 150, 32, 6
    rng, q, table, target = make(2, Q, N, D)
    excl = random_excl(rng, Q, N, target, 10)
    good = run(be, q, table, target, excl, k)
    assert good['err'] == 0
    bad_t = target.copy()
    bad_t[3], bad_t[66] = N, -1
    out = run(be, q, table, bad_t, excl, k)
    assert out['err'] & FLAG_BAD_INDEX
    keep = np.array([i for i in range(Q) if i not in (3, 66)])
    np.testing.assert_array_equal(out['rank'][keep], good['rank'][keep])
    np.testing.assert_array_equal(out['rows'], good['rows'])           # the top-k does not depend on the target
    assert out['rank'][3] == -1 and out['rank'][66] == -1
    bad_e = [list(e) for e in excl]
    bad_e[5] = bad_e[5] + [N + 7]                                       # (sorted: it is the largest)
    bad_e[9] = [-4] + bad_e[9]
    out = run(be, q, table, target, bad_e, k)
    assert out['err'] & FLAG_BAD_INDEX
    np.testing.assert_array_equal(out['rank'], good['rank'])
    np.testing.assert_array_equal(out['rows'], good['rows'])


def test_bad_excluded_row_is_flagged_without_targets(be):
    Q, N, D, k = 5, 40, 16, 4
    _, q, table, _ = make(4, Q, N, D)
    good = run(be, q, table, None, None, k)
    out = run(be, q, table, None, [[1, N]] + [[] for _ in range(Q - 1)], k)
    assert out['err'] & FLAG_BAD_INDEX
    np.testing.assert_array_equal(out['rows'][1:], good['rows'][1:])
    assert 1 not in out['rows'][0]
