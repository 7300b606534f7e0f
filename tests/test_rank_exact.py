"""The ranking kernels held to an exact oracle: integer scores, ties at every place of every list, non-finite rows.

Runs on the host fiber emulator (`emu`, no GPU needed) and on the gfx950 library (`hip`, marked gpu).

tests/test_rank.py, tests/test_rank_dot.py and tests/test_rank_mixed_kernels.py compare Gaussian data with float64 inside
a tolerance band, so the order "higher score first, the smaller row on equal scores" is only ever checked exactly on a
handful of hand-placed copies of one row. Here the operands are small integers: under score_kind 1 every product and every
partial sum of a dot is an integer below 2^24, exact in fp32 in any summation order, so the expected top-k rows, top-k
scores, ranks and target scores come out of int64 numpy and are compared with array_equal. A few dozen distinct scores
over thousands of rows tie at every place of every candidate list by themselves: at the k-th place, across the quarter
turns of a tile, across the tiles of a strip and across strips, between excluded and kept rows at once.

  oracle     s = q.astype(int64) @ table.astype(int64).T; eligible rows ordered by (-s, row);
             rank = 1 + #{eligible r != target: s[r] > s[t] or (s[r] == s[t] and r < t)}; expected scores float32(s);
             slots past the eligible rows hold -1 / -inf. Scores are compared by value: -0.0 is the score +0.0.
  cosine     rows of exactly four +-1 (norm 2) and queries of sixteen +-1 (norm 4): sqrtf and 1 / x of a power of two are
             exact under IEEE rounding, so score_kind 0 gives dot / 8 exactly; all-zero rows score 0.
  non-finite a NaN score counts as -inf (rank_score); among -inf scores the smaller row leads; a live -inf row keeps its
             row number (an empty slot is -1); +inf rows lead; target_scores of a NaN target is -inf, NaN being "no target".
  mixed      mpqe_rank_entities_mixed against the same oracle, not against the library's per-table call: a row is eligible
             when its `valid` bit is set and the query's exclusion bit is clear, both taken from the dense boolean arrays
             the bitmaps were packed from.

Every case asserts, from the oracle alone and before it calls the library: the (strips, tiles per strip) of rank_plan as
restated here (pinned to the library through the workspace size, which is a function of the strip count), abs(s).max() <
2^24, and for k >= 3 that at least half of the queries that have more than k eligible rows tie across the k-th place
(s[order[k - 1]] == s[order[k]]). References are built once per case (lru_cache) and shared by both backends.

Emulator time of the slowest cases: 3.6 s (test_the_query_block_term_of_the_plan) and 3.7 s (the mixed call at k = 128);
every other case stays under 1.2 s. No case is left to the device alone.
"""
import functools

import numpy as np
import pytest

from tests.fenced import fenced
from tests.test_rank import EPS, be, csr  # noqa: F401  (be: the emu / hip fixture)
from tests.test_rank_mixed_kernels import COUNTS, Problem, build, run_mixed

DOT, COSINE = 1, 0
TILE = 64                 # GT_BM = GT_BN
MAX_STRIPS = 64           # RANK_MAX_STRIPS
PIN_K = 128               # rank_plan does not read k; at 128 the list planes are whole 256-byte units per strip
NEG_INF = -np.inf


# ------------------------------------------------------------------------------------------ the plan, restated
def ceil_div(a, b):
    return -(-a // b)


def align_up(v, a=256):
    return ceil_div(v, a) * a


def plan(qblocks, tiles):
    """csrc/rank_core.h: rank_strip_rule, the one rule behind rank_plan (csrc/rank.hip) and rmx_plan (csrc/rank_mixed.hip)
    -> (S, tiles per strip of the widest table)"""
    want = max(1, min(ceil_div(768, qblocks), MAX_STRIPS, tiles))
    tps = ceil_div(tiles, want)
    return ceil_div(tiles, tps), tps


def pinned_plan(be, Q, N, D):
    """(S, tiles per strip) of one table's call; S is solved from the workspace size the library names."""
    S, tps = plan(ceil_div(Q, TILE), ceil_div(N, TILE))
    lists = be.lib.mpqe_rank_workspace_bytes(Q, N, D, PIN_K) - (align_up(N * 4) + 5 * align_up(Q * 4) + 256)
    assert lists % (2 * Q * PIN_K * 4) == 0 and lists // (2 * Q * PIN_K * 4) == S, 'the restated plan is not the library\'s'
    return S, tps


def pinned_mixed_plan(be, Q, rows, D):
    blocks = Q // TILE + len(rows)
    S, tps = plan(blocks, ceil_div(max(rows), TILE))
    fixed = 256 + 6 * align_up(Q * 4) + align_up(blocks * 16) + align_up(sum(rows) * 4)
    lists = be.lib.mpqe_rank_mixed_workspace_bytes(Q, len(rows), max(rows), sum(rows), D, PIN_K) - fixed
    assert lists % (2 * Q * PIN_K * 4) == 0 and lists // (2 * Q * PIN_K * 4) == S, 'the restated plan is not the library\'s'
    return S, tps


# ------------------------------------------------------------------------------------------ oracle
def i64(a):
    return a.astype(np.int64)


def f32(v):
    return np.asarray(v).astype(np.float32)


def eighth(v):
    return (np.asarray(v) / 8.0).astype(np.float32)          # (an integer / 8 is exact in float64 and in fp32)


def expected(s, k, target=None, banned=None, as_score=f32):
    """s [Q, N]: int64 dots, or float64 with +-inf where the score is not finite (a NaN score already -inf).
    banned [Q, N] bool or None. `judged`: the query has more than k eligible rows; `tied`: it ties across the k-th place."""
    Q, N = s.shape
    rowno = np.arange(N)
    out = {'rows': np.full((Q, k), -1, dtype=np.int64), 'scores': np.full((Q, k), NEG_INF, dtype=np.float32),
           'judged': np.zeros(Q, dtype=bool), 'tied': np.zeros(Q, dtype=bool)}
    if target is not None:
        out['rank'] = np.zeros(Q, dtype=np.int64)
        out['tscore'] = as_score(s[np.arange(Q), target])
    for i in range(Q):
        ok = np.ones(N, dtype=bool) if banned is None else ~banned[i]
        elig = rowno[ok]
        order = elig[np.argsort(-s[i, elig], kind='stable')]           # (-s, row): elig is in row order, the sort stable
        n = min(k, order.size)
        out['rows'][i, :n] = order[:n]
        out['scores'][i, :n] = as_score(s[i, order[:n]])
        if order.size > k:
            out['judged'][i] = True
            out['tied'][i] = s[i, order[k - 1]] == s[i, order[k]]
        if target is not None:
            t = int(target[i])
            ok[t] = False
            out['rank'][i] = 1 + int(((s[i] > s[i, t]) & ok).sum()) + int(((s[i] == s[i, t]) & ok & (rowno < t)).sum())
    return out


def assert_dense_ties(exp, k):
    """At least half of the queries with a k-th place inside their eligible rows tie across it (k >= 3)."""
    if k < 3 or not exp['judged'].any():
        return
    tied, judged = int(exp['tied'][exp['judged']].sum()), int(exp['judged'].sum())
    print('ties across place %d: %d of %d queries' % (k, tied, judged))
    assert 2 * tied >= judged, 'only %d of %d queries tie across place %d' % (tied, judged, k)


def assert_exact(out, exp, what=''):
    assert out['err'] == 0
    keys = ('rows', 'scores') + (('rank', 'tscore') if 'rank' in exp else ())
    for key in keys:
        np.testing.assert_array_equal(out[key], exp[key], err_msg='%s %s' % (what, key))


def run_scored(be, q, table, target, excl, k, kind=DOT, eps=EPS, mis_t=0):
    """One mpqe_rank_entities_scored call; q and table sit between NaN fences, the table `mis_t` floats off 16 bytes."""
    Q, D = q.shape
    N = table.shape[0]
    dq, dt = fenced(be, q), fenced(be, table, mis_t)
    dtarget = None if target is None else be.put(np.asarray(target, dtype=np.int64))
    off = rows = None
    E = 0
    if excl is not None:
        o, r = csr(excl, Q)
        E = int(r.shape[0])
        off, rows = be.put(o), be.put(r if E else np.zeros(1, dtype=np.int64))
    topr, tops = be.empty((Q, k), np.int64), be.empty((Q, k), np.float32)
    rank = be.empty((Q,), np.int64) if target is not None else None
    tsc = be.empty((Q,), np.float32) if target is not None else None
    need = be.lib.mpqe_rank_workspace_bytes(Q, N, D, k)
    ws = be.nbytes(need)
    err = be.zeros((1,), np.int32)
    st = be.lib.mpqe_rank_entities_scored(be.ptr(dq), Q, be.ptr(dt), N, D, eps, kind, be.ptr(dtarget), be.ptr(off),
                                          be.ptr(rows), E, k, be.ptr(topr), be.ptr(tops), be.ptr(rank), be.ptr(tsc),
                                          be.ptr(ws), need, be.ptr(err), be.stream)
    assert st == 0, 'status %d' % st
    get = lambda a: None if a is None else be.get(a)       # noqa: E731
    return {'rows': get(topr), 'scores': get(tops), 'rank': get(rank), 'tscore': get(tsc), 'err': int(be.get(err)[0])}


# ------------------------------------------------------------------------------------------ data
def small_ints(rng, shape):
    return rng.randint(-2, 3, size=shape).astype(np.float32)


def sparse_rows(rng, n, D, nnz, values):
    """n rows of D columns with exactly nnz entries drawn from `values`, the first and the last column among them on
    every other row (so that no column of the operand goes unread by every row)."""
    out = np.zeros((n, D), dtype=np.float32)
    for r in range(n):
        cols = rng.permutation(D)[:nnz]
        if r % 2 == 0 and nnz >= 2:
            cols = np.concatenate([[0, D - 1], 1 + rng.permutation(D - 2)[:nnz - 2]])
        out[r, cols] = rng.choice(values, size=cols.shape[0])
    return out


def edge_targets(rng, Q, N):
    """Random targets; the first ones sit on the last row, on both sides of the first tile boundary and on row 0."""
    target = rng.randint(0, N, size=Q).astype(np.int64)
    edges = [r for r in (N - 1, 64, 63, 0) if r < N][:Q]
    target[:len(edges)] = edges
    return target


def oracle_excl(rng, s, target, most=40):
    """Exclusion lists of up to `most` rows built from the oracle: the target itself on even queries, the oracle's best
    three rows on every third query (the head of the list changes), and the nearest row tied with the target on each side
    of it (an excluded row that precedes the target and one that does not, at the target's own score)."""
    Q, N = s.shape
    excl, both = [], 0
    for i in range(Q):
        t = int(target[i])
        rows = set(rng.choice(N, size=rng.randint(0, most - 5), replace=False).tolist())
        if i % 2 == 0:
            rows.add(t)
        if i % 3 == 0:
            rows.update(np.argsort(-s[i], kind='stable')[:3].tolist())
        same = np.nonzero(s[i] == s[i, t])[0]
        below, above = same[same < t], same[same > t]
        if below.size:
            rows.add(int(below[-1]))
        if above.size:
            rows.add(int(above[0]))
        both += 1 if below.size and above.size else 0
        assert len(rows) <= most
        excl.append(sorted(rows))
    assert both >= 1, 'no target has a tied row on each side'
    return excl


def banned_of(excl, N):
    out = np.zeros((len(excl), N), dtype=bool)
    for i, e in enumerate(excl):
        out[i, e] = True
    return out


@functools.lru_cache(maxsize=None)
def int_case(seed, Q, N, D, nnz=0):
    """Integer operands in [-2, 2] (queries with `nnz` non-zero entries when given; from five queries on the last one is
    all zeros), targets, oracle exclusion lists."""
    rng = np.random.RandomState(seed)
    table = small_ints(rng, (N, D))
    q = sparse_rows(rng, Q, D, nnz, [-2, -1, 1, 2]) if nnz else small_ints(rng, (Q, D))
    if Q >= 5:
        q[-1] = 0           # every row ties: the top-k is rows 0 .. k - 1, all of strip 0's first tile, whose full list must
    s = i64(q) @ i64(table).T       # turn away every later row of the strip -- at k = 16 and 64 with the variant's last entry
    assert np.abs(s).max() < 2 ** 24
    target = edge_targets(rng, Q, N)
    excl = oracle_excl(rng, s, target)
    return {'q': q, 'table': table, 's': s, 'target': target, 'excl': excl, 'banned': banned_of(excl, N)}


@functools.lru_cache(maxsize=None)
def int_expected(seed, Q, N, D, nnz, k, with_excl):
    c = int_case(seed, Q, N, D, nnz)
    return expected(c['s'], k, c['target'], c['banned'] if with_excl else None)


def check_int_case(be, seed, Q, N, D, k, with_excl, plan_is, nnz=0, mis_t=0):
    c = int_case(seed, Q, N, D, nnz)
    assert pinned_plan(be, Q, N, D) == plan_is
    assert np.abs(c['s']).max() < 2 ** 24
    exp = int_expected(seed, Q, N, D, nnz, k, with_excl)
    assert_dense_ties(exp, k)
    out = run_scored(be, c['q'], c['table'], c['target'], c['excl'] if with_excl else None, k, mis_t=mis_t)
    assert_exact(out, exp, 'Q %d N %d D %d k %d' % (Q, N, D, k))
    return c, exp


# ------------------------------------------------------------------------------------------ one table, score_kind 1
@pytest.mark.parametrize('with_excl', [False, True], ids=['plain', 'exclusions'])
@pytest.mark.parametrize('k', [1, 16, 17, 64, 65, 128])
def test_k_regimes_across_two_tiles_per_strip(be, k, with_excl):
    """N = 4161: 66 column tiles, 33 strips of two, the last tile one row wide. k = 16 and 64 fill the 16- and the 64-entry
    list variant exactly, 17 and 65 are the first k of the next one. 43 or so distinct scores over 4161 rows: the k-th
    place is tied in every query, and with it the early reject, the insertion behind equal scores, the carry of a full
    list into the strip's second tile and the merge of equal heads across strips. The last query is all zeros: its answer
    is rows 0 .. k - 1, so strip 0's list fills from its first rows and turns every later one away. The lists hold the target
    (even queries), the oracle's best three rows and a row tied with the target on each side of it."""
    c, exp = check_int_case(be, 11, 5, 4161, 8, k, with_excl, (33, 2))
    if with_excl:
        plain = int_expected(11, 5, 4161, 8, 0, k, False)
        assert (exp['rows'][:, 0] != plain['rows'][:, 0]).any(), 'no exclusion list changed the head of a list'
        assert (exp['rank'] != plain['rank']).any()


@pytest.mark.parametrize('k', [3, 16, 17, 32])
def test_one_strip_is_the_whole_list(be, k):
    """N = 64: one tile, one strip, so the k-th place of the strip's list IS the k-th place of the answer (with 33 strips
    of 128 rows an answer seldom reaches the last entry of a strip's list). D = 4: 17 or so distinct scores over 64 rows;
    a later row that equals the k-th entry must neither pass the scan nor displace it."""
    for with_excl in (False, True):
        check_int_case(be, 21, 70, 64, 4, k, with_excl, (1, 1))


def test_three_tiles_per_strip(be):
    """N = 8300: 130 tiles, 44 strips of three (the last strip holds one); k = 65 is the first k of the 128-entry lists."""
    for with_excl in (False, True):
        check_int_case(be, 12, 3, 8300, 8, 65, with_excl, (44, 3))


def test_two_query_blocks_the_second_partial(be):
    """Q = 70: a full block of 64 queries and one of 6, each with its own 33 strips; with exclusion lists."""
    check_int_case(be, 13, 70, 4161, 8, 17, True, (33, 2))


def test_the_query_block_term_of_the_plan(be):
    """Q = 3072: 48 query blocks, so the strip count comes from ceil(768 / 48) = 16 < 17 tiles: 9 strips of two tiles, the
    regime of an evaluation window of thousands of queries. 3.6 s on the emulator."""
    assert ceil_div(768, ceil_div(3072, TILE)) == 16 < ceil_div(1088, TILE)
    check_int_case(be, 14, 3072, 1088, 4, 5, False, (9, 2))


@pytest.mark.parametrize('D,mis_t,mode', [(32, 0, 'LD_FAST'), (20, 0, 'LD_PRED'), (10, 0, 'LD_SCALAR'), (32, 1, 'LD_SCALAR')],
                         ids=['D32_fast', 'D20_pred', 'D10_scalar', 'D32_table_4_bytes_off'])
def test_load_modes(be, D, mis_t, mode):
    """The three operand loaders of the tile core (whole 16-byte loads; predicated ones; element-wise ones, by the dim or
    by a table 4 bytes off alignment) give the oracle's answer exactly. The table is dense in [-2, 2]; a query has 8 non-zero
    entries, the first and the last column among them, which keeps the scores few enough to tie across the 10th place."""
    assert mode == ('LD_SCALAR' if (D % 4 or mis_t) else 'LD_FAST' if D % 32 == 0 else 'LD_PRED')
    for with_excl in (False, True):
        check_int_case(be, 15, 9, 4161, D, 10, with_excl, (33, 2), nnz=8, mis_t=mis_t)


# ------------------------------------------------------------------------------------------ one table, score_kind 0
def uniform_norm_table(rng, N, D, zero_every=97):
    table = sparse_rows(rng, N, D, 4, [-1, 1])
    table[::zero_every] = 0
    return table


@functools.lru_cache(maxsize=None)
def cosine_case(seed, Q, N, D):
    rng = np.random.RandomState(seed)
    table = uniform_norm_table(rng, N, D)
    q = sparse_rows(rng, Q, D, 16, [-1, 1])
    assert ((table * table).sum(axis=1) == np.where(np.arange(N) % 97 == 0, 0, 4)).all() and ((q * q).sum(axis=1) == 16).all()
    target = edge_targets(rng, Q, N)
    target[-1] = 97                                     # an all-zero row
    return {'q': q, 'table': table, 's': i64(q) @ i64(table).T, 'target': target}


def test_exact_cosine_with_zero_rows(be):
    """score_kind 0 on rows of norm 2 and queries of norm 4: the score is dot / 8 exactly (D = 80: rank_sumsq takes its
    second trip). Every 97th row is all zeros: it scores 0 (rank_row_inv) and ties with the orthogonal rows by row number.
    Nine distinct scores over 4161 rows, k = 65."""
    Q, N, D, k = 7, 4161, 80, 65
    c = cosine_case(16, Q, N, D)
    assert pinned_plan(be, Q, N, D) == (33, 2)
    assert np.abs(c['s']).max() < 2 ** 24
    exp = expected(c['s'], k, c['target'], None, as_score=eighth)
    assert_dense_ties(exp, k)
    assert (exp['tscore'][-1] == 0) and (c['s'][:, ::97] == 0).all()
    out = run_scored(be, c['q'], c['table'], c['target'], None, k, kind=COSINE)
    assert_exact(out, exp, 'cosine')


def test_zero_query_under_the_eps_clamp(be):
    """score_kind 0, one all-zero query: 1 / max(0, eps) is finite, so it scores exactly 0 against every row and ranks by
    row number; the other queries score dot / 8. eps = 1e30 scales every score of a query alike: same rows, same ranks,
    and the zero query still scores 0."""
    Q, N, D, k = 4, 300, 80, 20
    c = cosine_case(17, Q, N, D)
    q = c['q'].copy()
    q[2] = 0
    s = i64(q) @ i64(c['table']).T
    assert pinned_plan(be, Q, N, D) == (5, 1)
    assert np.abs(s).max() < 2 ** 24 and (s[2] == 0).all()
    exp = expected(s, k, c['target'], None, as_score=eighth)
    assert_dense_ties(exp, k)
    assert exp['rows'][2].tolist() == list(range(k)) and exp['rank'][2] == 1 + c['target'][2]
    out = run_scored(be, q, c['table'], c['target'], None, k, kind=COSINE, eps=1e-8)
    assert_exact(out, exp, 'eps 1e-8')
    big = run_scored(be, q, c['table'], c['target'], None, k, kind=COSINE, eps=1e30)
    assert big['err'] == 0
    np.testing.assert_array_equal(big['rows'], exp['rows'])
    np.testing.assert_array_equal(big['rank'], exp['rank'])
    assert (big['scores'][2] == 0).all() and big['tscore'][2] == 0


# ------------------------------------------------------------------------------------------ non-finite rows
@functools.lru_cache(maxsize=None)
def nonfinite_case(N, D):
    """Integer rows; NaN in one column of rows 0, 63, 64, 700 and N - 1; rows +inf * e0 and -inf * e0. Queries have a
    positive first component, except two all-zero ones (0 * inf is NaN); at D = 32 (whole 16-byte loads, whose clamped
    loads replicate the last row and the last query) the last query holds a NaN too."""
    rng = np.random.RandomState(18 + N + D)
    Q = 9
    nan_rows = sorted(set(r for r in (0, 63, 64, 700, N - 1) if r < N))
    pos_rows, neg_rows = [5, 66, N - 2], [6, 65, N - 3]
    clean = small_ints(rng, (N, D))
    q = sparse_rows(rng, Q, D, min(D, 8), [-2, -1, 1, 2])
    q[:, 0] = rng.randint(1, 3, size=Q)
    q[6:8] = 0
    clean[nan_rows + pos_rows + neg_rows] = 0
    table = clean.copy()
    for j, r in enumerate(nan_rows):
        table[r] = small_ints(rng, (D,))
        table[r, (3 * j + 1) % D] = np.nan
    table[pos_rows, 0] = np.inf
    table[neg_rows, 0] = -np.inf
    dots = i64(q) @ i64(clean).T
    assert np.abs(dots).max() < 2 ** 24
    s = dots.astype(np.float64)
    s[:, nan_rows] = NEG_INF                           # a NaN score ranks last
    s[:, pos_rows] = np.where(q[:, :1] > 0, np.inf, NEG_INF)       # (0 * inf: NaN)
    s[:, neg_rows] = NEG_INF
    if D == 32:
        q[8, 7] = np.nan
        s[8] = NEG_INF
    # targets: a NaN row, an inf row, a -inf row, an ordinary row, the last row (NaN), another NaN row; the zero queries on
    # an ordinary and on an inf row; the last query on an ordinary row
    target = np.array([63, 5, 6, 10, N - 1, nan_rows[-2], 10, 66, 20], dtype=np.int64)
    excl = []
    for i in range(Q):                                  # a NaN, an inf and a -inf row that precede some targets, and rows
        rows = set([0, 5, 6] + rng.choice(N, size=6, replace=False).tolist())       # at random
        if i % 2 == 0:
            rows.add(int(target[i]))
        excl.append(sorted(rows))
    return {'q': q, 'table': table, 's': s, 'target': target, 'excl': excl, 'banned': banned_of(excl, N), 'dots': dots}


@pytest.mark.parametrize('with_excl', [False, True], ids=['plain', 'exclusions'])
@pytest.mark.parametrize('D', [8, 32], ids=['D8_pred', 'D32_fast'])
@pytest.mark.parametrize('N,k', [(4161, 20), (70, 128)], ids=['N4161_k20', 'N70_k128'])
def test_non_finite_rows_and_queries(be, N, k, D, with_excl):
    """N = 70 with k = 128: k > N, every list reaches the -inf rows and then the empty slots. A live -inf row (NaN or -inf
    score) is returned with its row number, behind every finite score, the smaller row first; +inf rows lead; the zero
    queries tie every finite row at 0 in row order, with the inf rows at -inf; target_scores of a NaN target is -inf."""
    c = nonfinite_case(N, D)
    Q = c['q'].shape[0]
    assert pinned_plan(be, Q, N, D) == ((33, 2) if N == 4161 else (2, 1))
    assert np.abs(c['dots']).max() < 2 ** 24
    exp = expected(c['s'], k, c['target'], c['banned'] if with_excl else None)
    assert_dense_ties(exp, k)
    assert np.isneginf(exp['tscore'][[0, 2, 4, 5, 7]]).all() and exp['tscore'][1] == np.inf and exp['tscore'][6] == 0
    if not with_excl:
        assert exp['rows'][0, :3].tolist() == [5, 66, N - 2] and np.isposinf(exp['scores'][0, :3]).all()
        assert exp['rows'][6, :5].tolist() == [1, 2, 3, 4, 7]          # the zero query: rows 0, 5 and 6 are not finite
        if k > N:
            assert (exp['rows'][:, :N] >= 0).all() and np.isneginf(exp['scores'][:, N - 7:N]).all()        # (4 NaN + 3 -inf rows)
            assert (exp['rows'][:, N:] == -1).all()
            assert sorted(exp['rows'][6, :N].tolist()) == list(range(N))
    out = run_scored(be, c['q'], c['table'], c['target'], c['excl'] if with_excl else None, k)
    assert not np.isnan(out['scores']).any() and not np.isnan(out['tscore']).any()
    assert_exact(out, exp, 'N %d k %d D %d' % (N, k, D))


def test_negative_zero_ties_with_zero(be):
    """Products that underflow: -2^-100 * 2^-100 rounds to -0.0, and a dot whose every product is -0.0 or that underflow
    may come out as -0.0 where the next row's is +0.0 (D = 32: no zero padding of the K extent). Either is the score 0:
    the rows come in row order, over three strips. How many -0.0 arrived is printed, not asserted."""
    Q, N, D, k = 3, 130, 32, 128
    rng = np.random.RandomState(19)
    tiny = np.float32(2.0 ** -100)
    table = small_ints(rng, (N, D))
    table[::2] = np.abs(table[::2])                     # even rows: every product of query 0 is -0.0
    table[:, 0] = tiny * rng.randint(0, 3, size=N)
    q = np.zeros((Q, D), dtype=np.float32)
    q[0] = -0.0
    q[0, 0] = -tiny
    q[1, 0] = tiny
    q[2, 1:] = small_ints(rng, (D - 1,))
    s = i64(q[:, 1:]) @ i64(table[:, 1:]).T            # column 0 adds +-0 to every dot
    assert (s[:2] == 0).all() and np.abs(s).max() < 2 ** 24
    assert pinned_plan(be, Q, N, D) == (3, 1)
    target = np.array([129, 64, 63], dtype=np.int64)
    exp = expected(s, k, target)
    assert_dense_ties(exp, k)
    assert exp['rows'][0].tolist() == list(range(k)) and exp['rank'][:2].tolist() == [130, 65]
    out = run_scored(be, q, table, target, None, k)
    print('-0.0 among the scores of the two underflowing queries: %d of %d'
          % (int(np.signbit(out['scores'][:2]).sum()), 2 * k))
    assert_exact(out, exp, 'signed zeros')


# ------------------------------------------------------------------------------------------ the mixed call
MIX_ROWS = (1, 63, 64, 65, 4161)
MIX_D = 20
EDGE_ROWS = (0, 15, 16, 31, 32, 47, 48, 63, 64)
W_WIDE = ceil_div(max(MIX_ROWS), 32) + 2
W_NARROW = 40                                           # 1280 rows: rows past them are never excluded


def pack(dense):
    """[..., 32 * W] bool -> [..., W] int32 words, bit r % 32 of word r / 32 for row r"""
    lead = dense.shape[:-1]
    words = np.packbits(dense.reshape(lead + (-1, 32)), axis=-1, bitorder='little').view('<u4')
    return words.reshape(lead + (-1,)).view(np.int32)


@functools.lru_cache(maxsize=None)
def mixed_case(flip, W):
    """Five sets of integer tables. Kind 0 sets hold the uniform-norm rows (score dot / 8), kind 1 sets the same rows times
    1 or 2 (score dot: a kernel that took the other set's kind would return another number). Queries of sixteen +-1.
    `flip` swaps the kinds, which sets have a `valid` bitmap and the polarity of the valid bits at the edge rows."""
    rng = np.random.RandomState(20 + flip)
    shape = build(21, MIX_D, rows=MIX_ROWS, counts=COUNTS, with_bits=False, with_valid=False)     # groups, query -> set
    Q = shape.q.shape[0]
    qset = np.array([shape.set_of(i) for i in range(Q)])
    assert [int((qset == s).sum()) for s in range(5)] == list(COUNTS)
    kinds = [(s + flip) % 2 for s in range(5)]
    tables = []
    for s, n in enumerate(MIX_ROWS):
        t = uniform_norm_table(rng, n, MIX_D)
        tables.append(t * rng.randint(1, 3, size=(n, 1)).astype(np.float32) if kinds[s] == DOT else t)
    q = sparse_rows(rng, Q, MIX_D, 16, [-1, 1])
    edges = lambda n: [r for r in EDGE_ROWS + (n - 1,) if r < n]      # noqa: E731
    valid_dense = []
    for s, n in enumerate(MIX_ROWS):
        if s != 4 and (s + flip) % 2 == 0:
            valid_dense.append(None)
            continue
        ok = rng.rand(ceil_div(n, 32) * 32) < 0.8                      # holes; the last word's spare bits are random
        for j, r in enumerate(edges(n)):
            ok[r] = (j + s + flip) % 2 == 0
        valid_dense.append(ok)
    target = np.zeros(Q, dtype=np.int64)
    bits_dense = rng.rand(Q, W * 32) < 0.2
    for i in range(Q):
        s, n = int(qset[i]), MIX_ROWS[qset[i]]
        bits_dense[i, n:] = rng.rand(W * 32 - n) < 0.5 if n < W * 32 else False     # bits past the set's rows
        for j, r in enumerate(edges(n)):
            if r < W * 32:
                bits_dense[i, r] = (i + j) % 2 == 0
        target[i] = rng.randint(0, n)
        bad = None if valid_dense[s] is None else np.nonzero(~valid_dense[s][:n])[0]
        if i % 5 == 1 and bad is not None and bad.size:
            target[i] = bad[rng.randint(0, bad.size)]                  # a target whose valid bit is clear
        if i % 7 == 2:
            target[i] = n - 1
        if target[i] < W * 32 and i % 3 != 2:
            bits_dense[i, target[i]] = i % 3 == 0                      # the query's own target bit set / clear
    banned, dots = [], []
    for i in range(Q):
        s, n = int(qset[i]), MIX_ROWS[qset[i]]
        b = np.zeros(n, dtype=bool)
        m = min(n, W * 32)
        b[:m] = bits_dense[i, :m]
        if valid_dense[s] is not None:
            b |= ~valid_dense[s][:n]
        banned.append(b)
        dots.append(i64(q[i]) @ i64(tables[s]).T)
    pb = Problem(q, tables, kinds, [None if v is None else pack(v) for v in valid_dense], shape.set_of_group,
                 shape.group_of, target, pack(bits_dense))
    return {'pb': pb, 'qset': qset, 'banned': banned, 'dots': dots, 'valid_dense': valid_dense, 'bits_dense': bits_dense}


@functools.lru_cache(maxsize=None)
def mixed_expected(flip, W, k):
    c = mixed_case(flip, W)
    pb, qset = c['pb'], c['qset']
    Q = qset.shape[0]
    exp = {'rows': np.full((Q, k), -1, dtype=np.int64), 'scores': np.full((Q, k), NEG_INF, dtype=np.float32),
           'rank': np.zeros(Q, dtype=np.int64), 'tscore': np.zeros(Q, dtype=np.float32),
           'judged': np.zeros(Q, dtype=bool), 'tied': np.zeros(Q, dtype=bool)}
    for s in range(len(MIX_ROWS)):
        idx = np.nonzero(qset == s)[0]
        if idx.size == 0:
            continue
        part = expected(np.stack([c['dots'][i] for i in idx]), k, pb.target[idx], np.stack([c['banned'][i] for i in idx]),
                        as_score=eighth if pb.kinds[s] == COSINE else f32)
        for key in exp:
            exp[key][idx] = part[key]
    return exp


@pytest.mark.parametrize('k,W,flip', [(3, W_WIDE, 0), (17, W_NARROW, 1), (17, W_WIDE, 0), (128, W_WIDE, 1)],
                         ids=['k3_wide', 'k17_narrow_flipped', 'k17_wide', 'k128_wide_flipped'])
def test_mixed_call_against_the_integer_oracle(be, k, W, flip):
    """Sets of 1, 63, 64, 65 and 4161 rows, 0, 1, 64, 65 and 20 queries each, interleaved; 7 blocks at most, so 33 strips
    of two tiles for the widest set and one tile a strip for the others. Bitmaps with set and clear bits at rows 0, 15, 16,
    31, 32, 47, 48, 63, 64 and N - 1 (the 16-column quarters of a tile meet both halves of a 32-bit word), queries whose
    own target bit is set, targets whose valid bit is clear; the narrow exclusion width covers 1280 of the widest set's
    4161 rows. Ineligible rows are absent from the top-k and from the rank's count; the rest is exact."""
    c = mixed_case(flip, W)
    pb, qset = c['pb'], c['qset']
    Q = qset.shape[0]
    assert pinned_mixed_plan(be, Q, MIX_ROWS, MIX_D) == (33, 2)
    assert max(int(np.abs(d).max()) for d in c['dots']) < 2 ** 24
    assert (W * 32 < max(MIX_ROWS)) == (W == W_NARROW)
    # what the case was built to hold, read back from the dense arrays
    big = np.nonzero(qset == 4)[0]
    for r in EDGE_ROWS + (4160,):
        if r < W * 32:
            assert c['bits_dense'][big, r].any() and not c['bits_dense'][big, r].all()
    v = c['valid_dense'][4]
    assert v[list(EDGE_ROWS) + [4160]].any() and not v[list(EDGE_ROWS) + [4160]].all()
    own = c['bits_dense'][np.arange(Q), np.minimum(pb.target, W * 32 - 1)] & (pb.target < W * 32)
    assert own.any() and not own.all()
    assert any(c['valid_dense'][qset[i]] is not None and not c['valid_dense'][qset[i]][pb.target[i]] for i in range(Q))
    for i in range(0, Q, 7):                            # the dense arrays and the packed words say the same
        assert np.nonzero(c['banned'][i])[0].tolist() == pb.excluded(i)
    exp = mixed_expected(flip, W, k)
    assert_dense_ties(exp, k)
    out = run_mixed(be, pb, k)
    assert_exact(out, exp, 'mixed k %d W %d' % (k, W))
