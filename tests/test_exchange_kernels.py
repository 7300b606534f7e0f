"""The glue kernels of the data-parallel gradient exchange, one entry point at a time, against plain numpy: mpqe_spans_copy,
mpqe_rows_prepare, mpqe_rows_gather (csrc/p2p.hip), mpqe_rows_plan_build and mpqe_table_rows_sum (csrc/step.hip,
csrc/step_touch.h: table_sum_block; csrc/radix_sort.h), and mpqe_rgcn_general_aggregate (csrc/rgcn_general.hip). On the host
emulator and (gpu) on the real library, from one process: ranks are simulated by concatenation (an all-gather of fixed-size
slots is np.concatenate).

Everything is compared for exact equality -- the kernels copy, sort, or add floats in a documented order, so there is nothing
to round differently -- except two bounds derived from the addition order: the exchange's distance from the float64 sum
(test_row_exchange_of_simulated_ranks) and the aggregate's (_check_aggregate).

Every key handed to mpqe_rows_plan_build / mpqe_table_rows_sum is a (table << row_bits) | row inside its table, or ~0: they
trust their keys. Keys outside a table go to mpqe_rows_prepare alone, which masks them."""
import ctypes

import numpy as np
import pytest

from mpqe_amd._capi import STEP_MAX_MODES

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3          # include/mpqe_amd.h: MPQE_OK, MPQE_ERR_*
NOKEY = 2 ** 64 - 1                                           # csrc/step_touch.h: TOUCH_INVALID


@pytest.fixture(scope='module', params=['emu', pytest.param('hip', marks=pytest.mark.gpu)])
def be(request):
    from tests import kernel_backend
    return kernel_backend.EmuBackend() if request.param == 'emu' else kernel_backend.HipBackend()


def _a256(n):
    return (n + 255) // 256 * 256


def _at(be, host, misalign=0):
    """`host` on the backend, its first byte `misalign` bytes past a 256-byte boundary. A view of a larger allocation (which
    it keeps alive), so the pointer carries the offset."""
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


def _garbage(be, rng, nbytes):
    """nbytes (+ a little) of random bits, 256-byte aligned: a plan or a workspace before its build."""
    return _at(be, rng.randint(-2 ** 31, 2 ** 31 - 1, size=_a256(int(nbytes)) // 4 + 64).astype(np.int32))


def _bits(be, a):
    return np.ascontiguousarray(be.get(a)).view(np.uint32).copy()


def _u64(be, a):
    return np.ascontiguousarray(be.get(a)).view(np.uint64).copy()


def _put_keys(be, keys):
    """uint64 keys as the same 8 bytes of int64 (torch has no uint64 arithmetic to offer)"""
    return _at(be, np.ascontiguousarray(keys, dtype=np.uint64).view(np.int64))


def _ptrs(be, arrays):
    return (ctypes.c_void_p * len(arrays))(*[be.ptr(a) for a in arrays])


def _i64(*v):
    return (ctypes.c_int64 * len(v))(*v)


# ---------------------------------------------------------------------------------------------- mpqe_rows_plan_build
def _build_plan(be, d_keys, n, row_bits, key_bits, rng, keys=None):
    """-> (the plan on the backend, its bytes on the host); plan and workspace hold random bits when the build starts.
    keys: the host copy of d_keys -- the plan is compared with numpy's stable sort here, so that a kernel which indexes
    through its permutation is never launched on a wrong one."""
    pb = be.lib.mpqe_rows_plan_bytes(n)
    wb = be.lib.mpqe_rows_plan_workspace_bytes(n, key_bits)
    assert pb >= 256 + _a256(8 * n) + _a256(4 * n) and wb > 0
    plan, ws = _garbage(be, rng, pb), _garbage(be, rng, wb)
    be.check(be.lib.mpqe_rows_plan_build(be.ptr(d_keys), n, row_bits, key_bits, be.ptr(plan), pb, be.ptr(ws), wb, be.stream),
             'rows plan')
    host = np.ascontiguousarray(be.get(plan)).view(np.uint8).copy()          # (the build has run before `ws` goes away)
    if keys is not None:
        M, rb, _, _, skeys, perm = _read_plan(host, n)
        order = np.argsort(keys, kind='stable')
        assert (M, rb) == (n, row_bits)
        np.testing.assert_array_equal(perm, order.astype(np.int32))
        np.testing.assert_array_equal(skeys, keys[order])
    return plan, host


def _read_plan(host, n):
    """header {int64 M, int32 row_bits, int32 key_bits, 12 more words} at 0, keys [n] u64 at 256, perm [n] i32 behind them"""
    M = int(host[:8].view(np.int64)[0])
    words = host[8:64].view(np.int32)
    keys = host[256:256 + 8 * n].view(np.uint64)
    perm = host[256 + _a256(8 * n):256 + _a256(8 * n) + 4 * n].view(np.int32)
    return M, int(words[0]), int(words[1]), words[2:], keys, perm


@pytest.mark.parametrize('row_bits,key_bits', [(3, 8), (11, 16), (19, 24), (27, 32), (35, 40), (40, 45)])
def test_rows_plan_is_numpys_stable_sort(be, row_bits, key_bits):
    """1 to 6 passes of 8 bits: with an even count the first pass lands in the scratch pair, not in the output
    (radix_sort.h: to_out). n: one item, partial waves (63, 65, 255), exactly one tile of 2048, one item more (two
    workgroups: the scan over 256 * nblk counters, a last workgroup with one item), four workgroups with a ragged last."""
    for n in (1, 63, 64, 65, 255, 2047, 2048, 2049, 6200):
        rng = np.random.RandomState(1000 * key_bits + n)
        pool = np.unique(rng.randint(0, 2 ** key_bits - 1, size=max(1, n // 3), dtype=np.int64)).astype(np.uint64)
        keys = pool[rng.randint(0, len(pool), size=n)]
        keys[rng.rand(n) < 0.05] = NOKEY
        if n == 6200:
            assert len(np.unique(keys)) < n // 2 and (keys == NOKEY).any() and (keys != NOKEY).any()
        d_keys = _put_keys(be, keys)
        plan, host = _build_plan(be, d_keys, n, row_bits, key_bits, rng)
        M, rb, kb, rest, skeys, perm = _read_plan(host, n)
        assert (M, rb, kb) == (n, row_bits, key_bits), 'header, n = %d' % n
        assert not rest.any(), 'header padding (word 0: the "could not be built" mark), n = %d' % n
        order = np.argsort(keys, kind='stable')
        np.testing.assert_array_equal(perm, order.astype(np.int32), err_msg='permutation, n = %d' % n)
        np.testing.assert_array_equal(skeys, keys[order], err_msg='sorted keys, n = %d' % n)


# ---------------------------------------------------------------------------------------------- mpqe_table_rows_sum
SUM_ROWS = (300, 200)
SUM_ROW_BITS = 12
RUNS = (1, 2, 8, 9, 10, 16, 17, 18, 24, 25, 26, 33, 40, 1, 1, 9)
# (runs, trailing ~0 keys): table_sum_block requests TS_AHEAD = 8 positions behind a run's first and takes the rest in chunks
# of 8 -- runs that end inside the look-ahead (<= 9), exactly on a chunk boundary (9, 17, 25, 33), one behind and one before;
# the last run ends at M - 1 (tail 0: the clamp j < M ? j : M - 1), one position before it, or in front of nine ~0 keys
SUM_PLANS = [(RUNS, 0), (RUNS, 1), (RUNS, 9), ((1,), 0), ((9,), 0), ((17,), 0)]


def _run_keys(rng, runs, tail):
    """keys of distinct (table, row) pairs, the i-th smallest repeated runs[i] times, + `tail` times ~0; shuffled (the plan's
    stable sort puts them back in run order, members in input order)"""
    flat = np.sort(rng.choice(sum(SUM_ROWS), size=len(runs), replace=False))
    if len(runs) == len(RUNS):
        assert flat[0] < SUM_ROWS[0] <= flat[-1]                      # both tables
    distinct = np.where(flat < SUM_ROWS[0], flat, (1 << SUM_ROW_BITS) | (flat - SUM_ROWS[0])).astype(np.uint64)
    keys = np.concatenate([np.repeat(distinct, runs), np.full(tail, NOKEY, dtype=np.uint64)])
    return keys[rng.permutation(len(keys))]


def _sum_reference(keys, rows, tables, row_bits, store):
    """per key: acc = rows[first], then acc = float32(acc + rows[next]) in input order; row = acc / float32(row + acc)"""
    out = [None if t is None else t.copy() for t in tables]
    for key in np.unique(keys):
        if int(key) == NOKEY:
            continue
        members = np.flatnonzero(keys == key)
        acc = rows[members[0]].copy()
        for i in members[1:]:
            acc = (acc + rows[i]).astype(np.float32)
        t, r = int(key) >> row_bits, int(key) & ((1 << row_bits) - 1)
        assert t < len(tables) and r < SUM_ROWS[t]
        if out[t] is not None:
            out[t][r] = acc if store else (out[t][r] + acc).astype(np.float32)
    return out


def _sum_call(be, plan, n, d_rows, D, d_tabs, store, num_modes=None):
    tabs = _ptrs(be, d_tabs)
    return be.lib.mpqe_table_rows_sum(be.ptr(plan), n, be.ptr(d_rows), D, tabs, len(d_tabs) if num_modes is None else num_modes,
                                      store, be.stream)


@pytest.mark.parametrize('store', [0, 1], ids=['add', 'store'])
@pytest.mark.parametrize('D', [4, 16, 64, 128, 256, 1024])
def test_table_rows_sum_run_lengths(be, D, store):
    """D = 4: one lane a position, 256 positions a workgroup (the whole plan in one); D = 1024: one position a workgroup.
    Whole tables bit for bit: the rows no key names keep theirs."""
    for pi, (runs, tail) in enumerate(SUM_PLANS):
        rng = np.random.RandomState(97 * pi + D + store)
        keys = _run_keys(rng, runs, tail)
        n = len(keys)
        rows = rng.randn(n, D).astype(np.float32)
        tables = [rng.randn(r, D).astype(np.float32) for r in SUM_ROWS]
        want = _sum_reference(keys, rows, tables, SUM_ROW_BITS, store)
        d_keys = _put_keys(be, keys)
        plan, _ = _build_plan(be, d_keys, n, SUM_ROW_BITS, SUM_ROW_BITS + 5, rng, keys)
        d_rows = _at(be, rows)
        d_tabs = [_at(be, t) for t in tables]
        assert _sum_call(be, plan, n, d_rows, D, d_tabs, store) == OK
        for t in range(2):
            np.testing.assert_array_equal(_bits(be, d_tabs[t]), want[t].view(np.uint32),
                                          err_msg='runs %r + %d invalid keys, table %d' % (runs, tail, t))
        np.testing.assert_array_equal(_bits(be, d_rows), rows.view(np.uint32))            # (read only)


@pytest.mark.parametrize('store', [0, 1], ids=['add', 'store'])
def test_table_rows_sum_without_one_table(be, store):
    """table 1's pointer is NULL in the host array: its keys are dropped, table 0 gets the bits it gets beside table 1"""
    D = 64
    rng = np.random.RandomState(5)
    keys = _run_keys(rng, RUNS, 1)
    n = len(keys)
    rows = rng.randn(n, D).astype(np.float32)
    tables = [rng.randn(r, D).astype(np.float32) for r in SUM_ROWS]
    want = _sum_reference(keys, rows, tables, SUM_ROW_BITS, store)
    assert (want[1] != tables[1]).any()
    d_keys = _put_keys(be, keys)
    plan, _ = _build_plan(be, d_keys, n, SUM_ROW_BITS, SUM_ROW_BITS + 5, rng, keys)
    d_rows = _at(be, rows)
    d_tab0, d_tab1 = _at(be, tables[0]), _at(be, tables[1])
    assert _sum_call(be, plan, n, d_rows, D, [d_tab0, None], store) == OK
    np.testing.assert_array_equal(_bits(be, d_tab0), want[0].view(np.uint32))
    np.testing.assert_array_equal(_bits(be, d_tab1), tables[1].view(np.uint32))


# ---------------------------------------------------------------------------------------------- the whole row exchange
X_ROWS = (700, 5, 300)
X_BASE = (0, 700, 705)                  # the flat view [sum of rows, D]: row_base = the running sum
X_ROW_BITS = 10
X_HOT = ((0, 3), (0, 77), (0, 699), (1, 2), (2, 1), (2, 299))          # rows that EVERY rank touches


def _xkey(t, r):
    return (t << X_ROW_BITS) | r


def _rank_keys(rng, rank):
    """The sorted keys of one rank's touch plan, as a step leaves them: repeats; the hot rows; rank 0 more than 256 entries
    with a run across positions 255 | 256 (two workgroups of mpqe_rows_prepare); rank 1 nothing but the hot rows; what a
    plan may hold after a failed in-step sort: a row one past its table's last and one far beyond, a table that does not
    exist; two trailing ~0."""
    keys = np.repeat([_xkey(t, r) for t, r in X_HOT], rng.randint(1, 4, size=len(X_HOT))).tolist()
    if rank != 1:
        m = 330 if rank == 0 else int(rng.randint(20, 200))
        for f in rng.randint(0, sum(X_ROWS), size=m):
            t = 0 if f < X_BASE[1] else 1 if f < X_BASE[2] else 2
            keys.append(_xkey(t, int(f) - X_BASE[t]))
    keys += [_xkey(1, X_ROWS[1]), _xkey(1, 900), _xkey(9, 0)]
    keys = np.sort(np.array(keys, dtype=np.uint64))
    if rank == 0:
        keys[254:258] = keys[254]                                   # (still sorted: a run of >= 4 from position 254)
        t, r = int(keys[254]) >> X_ROW_BITS, int(keys[254]) & 1023
        assert len(keys) > 256 and t < 3 and r < X_ROWS[t] and keys[255] == keys[256]
    assert all(np.uint64(_xkey(t, r)) in keys for t, r in X_HOT)
    return np.concatenate([keys, np.full(2, NOKEY, dtype=np.uint64)])


def _prepare_reference(keys, cap):
    """the first key of every run goes out if it names a row of a table; every other slot, and M .. cap, ~0 with row 0"""
    send = np.full(cap, NOKEY, dtype=np.uint64)
    gidx = np.zeros(cap, dtype=np.int64)
    for i in range(len(keys)):
        k = int(keys[i])
        if (i > 0 and int(keys[i - 1]) == k) or k == NOKEY:
            continue
        t, r = k >> X_ROW_BITS, k & ((1 << X_ROW_BITS) - 1)
        if t < len(X_ROWS) and r < X_ROWS[t]:
            send[i] = k
            gidx[i] = X_BASE[t] + r
    return send, gidx


def _final_sum(be, all_keys, all_rows, D, rng):
    """plan over every rank's keys + the sum into tables pre-filled with 3.0 -> the flat [rows, D] view's bits"""
    n = len(all_keys)
    d_keys = _put_keys(be, all_keys)
    plan, _ = _build_plan(be, d_keys, n, X_ROW_BITS, X_ROW_BITS + 5, rng, all_keys)
    d_rows = _at(be, all_rows)
    d_tabs = [_at(be, np.full((r, D), 3.0, dtype=np.float32)) for r in X_ROWS]
    assert _sum_call(be, plan, n, d_rows, D, d_tabs, 1) == OK
    return np.concatenate([_bits(be, t) for t in d_tabs])


@pytest.mark.parametrize('D', [16, 128])
@pytest.mark.parametrize('world', [2, 8, 16])
def test_row_exchange_of_simulated_ranks(be, world, D):
    """include/mpqe_amd.h: "the same additions in the same order on every rank -- equal to the dense all-reduce". Per rank
    mpqe_rows_prepare + mpqe_rows_gather against plain loops; then the plan over all ranks' slots and the sum: every row
    some rank sent = the float32 sum of those ranks' gradient rows in rank order, bit for bit; every other row untouched.
    At world 16 the hot rows' runs are 16 long: the chunk loop of table_sum_block."""
    rng = np.random.RandomState(100 * world + D)
    total = sum(X_ROWS)
    rank_keys = [_rank_keys(rng, r) for r in range(world)]
    sizes = [len(k) for k in rank_keys]
    assert len(set(sizes)) > world // 2                              # (M differs between ranks)
    cap = max(sizes) + 37
    grads = [rng.randn(total, D).astype(np.float32) for _ in range(world)]
    table_rows, row_base = _i64(*X_ROWS), _i64(*X_BASE)
    sent_keys, sent_rows, sent_gidx = [], [], []
    for r in range(world):
        keys, M = rank_keys[r], sizes[r]
        want_send, want_gidx = _prepare_reference(keys, cap)
        assert (want_send != NOKEY).sum() >= len(X_HOT)
        d_keys = _put_keys(be, keys)
        d_send, d_gidx = be.empty((cap,), np.int64), be.empty((cap,), np.int64)
        assert be.lib.mpqe_rows_prepare(be.ptr(d_keys), M, cap, X_ROW_BITS, table_rows, row_base, len(X_ROWS), be.ptr(d_send),
                                        be.ptr(d_gidx), be.stream) == OK
        send, gidx = _u64(be, d_send), be.get(d_gidx)
        np.testing.assert_array_equal(send, want_send, err_msg='send_keys of rank %d' % r)
        np.testing.assert_array_equal(gidx, want_gidx, err_msg='gidx of rank %d' % r)
        d_grad = _at(be, grads[r])
        d_out = _at(be, np.full((cap + 1, D), np.nan, dtype=np.float32))       # (+ a guard row)
        assert be.lib.mpqe_rows_gather(be.ptr(d_grad), be.ptr(d_gidx), cap, D, be.ptr(d_out), be.stream) == OK
        out = be.get(d_out)
        np.testing.assert_array_equal(out[:cap].view(np.uint32), grads[r][want_gidx].view(np.uint32),
                                      err_msg='gathered rows of rank %d' % r)
        assert np.isnan(out[cap]).all(), 'mpqe_rows_gather wrote behind row n - 1'
        sent_keys.append(send)
        sent_rows.append(out[:cap].copy())
        sent_gidx.append(gidx)
    only_hot = set(sent_gidx[1][sent_keys[1] != NOKEY].tolist())
    assert only_hot == set(X_BASE[t] + r for t, r in X_HOT)          # rank 1 sends the hot rows and nothing else

    all_keys, all_rows = np.concatenate(sent_keys), np.concatenate(sent_rows)
    got = _final_sum(be, all_keys, all_rows, D, rng)

    want = np.full((total, D), 3.0, dtype=np.float32)
    ref64, mag64 = np.zeros((total, D)), np.zeros((total, D))
    count = np.zeros(total, dtype=np.int64)
    for r in range(world):
        for row in sent_gidx[r][sent_keys[r] != NOKEY]:
            g = grads[r][row]
            want[row] = g if count[row] == 0 else (want[row] + g).astype(np.float32)
            ref64[row] += g.astype(np.float64)
            mag64[row] += np.abs(g.astype(np.float64))
            count[row] += 1
    hot = [X_BASE[t] + r for t, r in X_HOT]
    assert (count[hot] == world).all() and (count == 0).any() and count.max() == world
    np.testing.assert_array_equal(got, want.view(np.uint32))         # (rows nobody sent: still exactly 3.0)
    # float32 summation of `count` terms in a fixed order: |error| <= (count - 1) u sum |g|, u = 2^-24; world >= count
    err = np.abs(got.view(np.float32).astype(np.float64) - ref64)[count > 0]
    assert (err <= (world - 1) * 2.0 ** -24 * mag64[count > 0]).all()
    if world == 8:      # a second replica: its own plan from the ranks concatenated in the same order -> the same bytes
        again = _final_sum(be, np.concatenate(sent_keys), np.concatenate(sent_rows), D, np.random.RandomState(1))
        np.testing.assert_array_equal(again, got)


# ---------------------------------------------------------------------------------------------- mpqe_spans_copy
SPANS = (1, 3, 4, 5, 4095, 4096, 4097, 8192, 8193, 7, 12289)


def _span_layout(rng, lengths):
    """[(dst offset, src offset, floats)], sizes of both buffers: a gap of 0 .. 3 floats before every span on either side,
    the source's first span from float offset 1 on"""
    recs, d, s = [], 0, 1
    for n in lengths:
        d += int(rng.randint(0, 4))
        s += int(rng.randint(0, 4))
        recs.append((d, s, int(n)))
        d += int(n)
        s += int(n)
    return recs, d + 9, s + 5


def _span_table(be, recs, back=False):
    """device records {dst, src, n, first_block} int64, first_block = the running sum of ceil(n / 4096); back: mirrored"""
    tab, blk = [], 0
    for d, s, n in recs:
        tab.append((s, d, n, blk) if back else (d, s, n, blk))
        blk += (n + 4095) // 4096
    return _at(be, np.array(tab, dtype=np.int64)), blk


def _check_spans(be, rng, lengths):
    recs, nd, ns = _span_layout(rng, lengths)
    # 16-byte form (both ends of a span on 16-byte boundaries) and scalar form both occur
    aligned = [n for d, s, n in recs if d % 4 == 0 and s % 4 == 0]
    assert 0 < len(aligned) < len(recs)
    src = rng.randn(ns).astype(np.float32)
    want = np.full(nd, 7.0, dtype=np.float32)
    for d, s, n in recs:
        want[d:d + n] = src[s:s + n]
    d_src, d_dst = _at(be, src), _at(be, np.full(nd, 7.0, dtype=np.float32))
    table, blocks = _span_table(be, recs)
    assert be.lib.mpqe_spans_copy(be.ptr(d_dst), be.ptr(d_src), be.ptr(table), len(recs), blocks, be.stream) == OK
    np.testing.assert_array_equal(_bits(be, d_dst), want.view(np.uint32))          # (gaps and tail: still 7.0)
    np.testing.assert_array_equal(_bits(be, d_src), src.view(np.uint32))
    # and back through the mirrored table, as parallel.py does with spans_out: the spans of the source again
    back = np.full(ns, -2.0, dtype=np.float32)
    for d, s, n in recs:
        back[s:s + n] = src[s:s + n]
    d_back = _at(be, np.full(ns, -2.0, dtype=np.float32))
    table_out, blocks_out = _span_table(be, recs, back=True)
    assert blocks_out == blocks
    assert be.lib.mpqe_spans_copy(be.ptr(d_back), be.ptr(d_dst), be.ptr(table_out), len(recs), blocks, be.stream) == OK
    np.testing.assert_array_equal(_bits(be, d_back), back.view(np.uint32))
    return aligned


def test_spans_copy_edges(be):
    """spans of one workgroup less one float, exactly one, one float more, two and three workgroups; tails of 1 to 3 floats;
    16-byte aligned pairs and pairs that are not"""
    aligned = []
    for seed in (6, 11, 24, 27):          # (one span in sixteen starts on 16-byte boundaries at both ends: four layouts)
        aligned += _check_spans(be, np.random.RandomState(seed), SPANS)
    # the 16-byte form with whole workgroups, with a scalar tail of 1 and of 3 floats, and with a tail in a later workgroup
    assert set(aligned) >= {8192, 5, 7, 4095, 8193}


def test_spans_copy_many_spans(be):
    """300 spans of 1 to 9000 floats, up to three workgroups each: the search over first_block"""
    rng = np.random.RandomState(3)
    _check_spans(be, rng, rng.randint(1, 9001, size=300))


# ---------------------------------------------------------------------------------------------- mpqe_rgcn_general_aggregate
AGG = dict(Nn=60, E=400, R=5)


def _agg_graph(rng):
    """duplicate edges, self loops, nodes 50 .. 59 without in-edges, ~110 edges into node 7, relation 3 unused"""
    Nn, E = AGG['Nn'], AGG['E']
    src, dst = rng.randint(0, Nn, size=E), rng.randint(0, 50, size=E)
    et = rng.choice([0, 1, 2, 4], size=E)
    dst[:100] = 7
    src[100:110] = dst[100:110]
    src[110:120], dst[110:120], et[110:120] = src[120:130], dst[120:130], et[120:130]
    order = rng.permutation(E)
    return np.stack([src[order], dst[order]]).astype(np.int64), et[order].astype(np.int64)


def _agg_plan(be, ei, et):
    Nn, E, R = AGG['Nn'], AGG['E'], AGG['R']
    pb, pw = be.lib.mpqe_rgcn_plan_bytes(Nn, E, R), be.lib.mpqe_rgcn_plan_workspace_bytes(Nn, E, R)
    plan, ws, err = be.nbytes(pb), be.nbytes(pw), be.zeros((1,), np.int32)
    d_ei, d_et = be.put(ei), be.put(et)
    be.check(be.lib.mpqe_rgcn_plan_build(be.ptr(d_ei), be.ptr(d_et), Nn, E, R, be.ptr(plan), pb, be.ptr(ws), pw, be.ptr(err),
                                         be.stream), 'plan')
    assert int(be.get(err)[0]) == 0
    return plan


def _check_aggregate(be, dim, with_bias, relu, misalign):
    """out[i] = act(bias + msg[E + i] + sum of the rows of the edges into i) against float64. An edge's message row is its
    position in the relation-sorted order, which is the STABLE sort by edge_type (what the plan's radix sort gives).
    |error| <= (indegree + 2) 2^-24 (|bias| + |self| + sum |rows|) per element: float32 additions in any one order. With
    relu an element whose float64 value is that close to zero may come out as 0 or as the small value; fewer than 1 % of
    the elements may be such (Gaussian inputs: far fewer are)."""
    Nn, E, R = AGG['Nn'], AGG['E'], AGG['R']
    rng = np.random.RandomState(40 + dim + misalign)
    ei, et = _agg_graph(rng)
    indeg = np.bincount(ei[1], minlength=Nn)
    assert indeg.max() >= 100 and (indeg == 0).sum() >= 10 and (ei[0] == ei[1]).any() and 3 not in et
    assert len(set(zip(ei[0].tolist(), ei[1].tolist(), et.tolist()))) < E
    msg = rng.randn(E + Nn, dim).astype(np.float32)
    bias = rng.randn(dim).astype(np.float32) if with_bias else None
    pos = np.empty(E, dtype=np.int64)
    pos[np.argsort(et, kind='stable')] = np.arange(E)
    m64 = msg.astype(np.float64)
    ref = m64[E:] + (bias.astype(np.float64) if with_bias else 0.0)
    mag = np.abs(m64[E:]) + (np.abs(bias.astype(np.float64)) if with_bias else 0.0)
    np.add.at(ref, ei[1], m64[pos])
    np.add.at(mag, ei[1], np.abs(m64[pos]))
    bound = (indeg[:, None] + 2) * 2.0 ** -24 * mag

    plan = _agg_plan(be, ei, et)
    d_msg = _at(be, msg)
    d_bias = _at(be, bias) if with_bias else None
    d_buf = _at(be, np.full((Nn + 2, dim), np.nan, dtype=np.float32), misalign)          # a guard row on either side
    d_out = d_buf[1:]
    assert be.lib.mpqe_rgcn_general_aggregate(be.ptr(plan), Nn, E, R, be.ptr(d_msg), be.ptr(d_bias), dim, relu, be.ptr(d_out),
                                              be.stream) == OK
    buf = be.get(d_buf)
    assert np.isnan(buf[0]).all() and np.isnan(buf[Nn + 1]).all(), 'the aggregate wrote outside out[0 .. Nn)'
    got = buf[1:Nn + 1].astype(np.float64)
    if not relu:
        assert (np.abs(got - ref) <= bound).all()
        return
    near = np.abs(ref) <= bound
    assert near.sum() < 0.01 * near.size
    assert (np.abs(got - np.maximum(ref, 0.0)) <= bound)[~near].all()
    assert ((got == 0.0) | (np.abs(got - ref) <= bound))[near].all()
    assert (got >= 0.0).all()


@pytest.mark.parametrize('case', [(64, True, 1, 0), (20, False, 0, 0), (10, True, 0, 0), (64, True, 1, 4)],
                         ids=['dim64_bias_relu', 'dim20_no_bias', 'dim10_scalar', 'dim64_out_plus4bytes'])
def test_general_aggregate_vs_float64(be, case):
    """dim 64 / 20: 16 bytes a lane; dim 10, and dim 64 with `out` 4 bytes past its boundary: the scalar form"""
    _check_aggregate(be, *case)


def test_general_aggregate_of_no_nodes(be):
    """num_nodes = 0: OK, and nothing is written"""
    rng = np.random.RandomState(8)
    ei, et = _agg_graph(rng)
    plan = _agg_plan(be, ei, et)
    d_msg = _at(be, rng.randn(AGG['E'], 64).astype(np.float32))
    d_out = _at(be, np.full((4, 64), np.nan, dtype=np.float32))
    assert be.lib.mpqe_rgcn_general_aggregate(be.ptr(plan), 0, AGG['E'], AGG['R'], be.ptr(d_msg), None, 64, 1, be.ptr(d_out),
                                              be.stream) == OK
    assert np.isnan(be.get(d_out)).all()


# ---------------------------------------------------------------------------------------------- argument checks
def test_spans_copy_argument_checks(be):
    src = np.arange(64, dtype=np.float32)
    d_src, d_dst = _at(be, src), _at(be, np.full(64, 7.0, dtype=np.float32))
    table, blocks = _span_table(be, [(0, 0, 64)])
    args = (be.ptr(d_dst), be.ptr(d_src), be.ptr(table), 1, blocks)
    for i, bad in ((0, None), (1, None), (2, None), (3, 0), (3, -1), (4, 0), (4, -1), (4, 2 ** 31)):
        call = args[:i] + (bad,) + args[i + 1:]
        assert be.lib.mpqe_spans_copy(*(call + (be.stream,))) == INVALID, 'argument %d = %r' % (i, bad)
    np.testing.assert_array_equal(be.get(d_dst), np.full(64, 7.0, dtype=np.float32))
    assert be.lib.mpqe_spans_copy(*(args + (be.stream,))) == OK
    np.testing.assert_array_equal(be.get(d_dst), src)


def test_rows_prepare_argument_checks(be):
    keys = np.array([_xkey(0, 1), _xkey(0, 1), _xkey(2, 5), NOKEY], dtype=np.uint64)
    M, cap = len(keys), len(keys) + 3
    d_keys = _put_keys(be, keys)
    d_send, d_gidx = be.empty((cap,), np.int64), be.empty((cap,), np.int64)
    table_rows, row_base = _i64(*X_ROWS), _i64(*X_BASE)
    many = STEP_MAX_MODES + 1
    rows_many, base_many = _i64(*([4] * many)), _i64(*range(0, 4 * many, 4))

    def call(M=M, cap=cap, row_bits=X_ROW_BITS, num_tables=len(X_ROWS), keys=d_keys, send=d_send, gidx=d_gidx, rows=table_rows,
             base=row_base):
        return be.lib.mpqe_rows_prepare(be.ptr(keys), M, cap, row_bits, rows, base, num_tables, be.ptr(send), be.ptr(gidx),
                                        be.stream)
    assert call(M=-1) == INVALID
    assert call(cap=M - 1) == INVALID
    assert call(M=0, cap=0) == INVALID
    assert call(row_bits=0) == INVALID
    assert call(row_bits=41) == INVALID
    assert call(num_tables=0) == INVALID
    assert call(num_tables=many, rows=rows_many, base=base_many) == INVALID
    assert call(keys=None) == INVALID
    assert call(send=None) == INVALID
    assert call(gidx=None) == INVALID
    assert call(rows=None) == INVALID
    assert call(base=None) == INVALID
    for out in (d_send, d_gidx):
        np.testing.assert_array_equal(be.get(out), np.full(cap, -7, dtype=np.int64))
    assert call() == OK
    want_send, want_gidx = _prepare_reference(keys, cap)
    np.testing.assert_array_equal(_u64(be, d_send), want_send)
    np.testing.assert_array_equal(be.get(d_gidx), want_gidx)
    # M = 0 is a plan without entries: every slot goes out invalid
    assert call(M=0) == OK
    np.testing.assert_array_equal(_u64(be, d_send), np.full(cap, NOKEY, dtype=np.uint64))
    np.testing.assert_array_equal(be.get(d_gidx), np.zeros(cap, dtype=np.int64))


def test_rows_gather_argument_checks(be):
    rng = np.random.RandomState(4)
    n = 5
    rows = rng.randn(9, 8).astype(np.float32)
    d_rows = _at(be, np.concatenate([rows.ravel(), np.zeros(4, dtype=np.float32)]))
    d_out = _at(be, np.full(n * 8 + 4, np.nan, dtype=np.float32))
    d_rows4, d_out4 = d_rows[1:], d_out[1:]                         # 4 bytes past the boundary
    gidx = np.array([8, 0, 3, 3, 7], dtype=np.int64)
    d_gidx = _at(be, gidx)

    def call(rows=d_rows, gidx=d_gidx, n=n, dim=8, out=d_out):
        return be.lib.mpqe_rows_gather(be.ptr(rows), be.ptr(gidx), n, dim, be.ptr(out), be.stream)
    assert call(n=0) == INVALID
    assert call(n=-1) == INVALID
    assert call(dim=6) == INVALID
    assert call(dim=0) == INVALID
    assert call(rows=d_rows4) == INVALID
    assert call(out=d_out4) == INVALID
    assert call(rows=None) == INVALID
    assert call(gidx=None) == INVALID
    assert call(out=None) == INVALID
    assert np.isnan(be.get(d_out)).all()
    assert call() == OK
    out = be.get(d_out)
    np.testing.assert_array_equal(out[:n * 8].reshape(n, 8), rows[gidx])
    assert np.isnan(out[n * 8:]).all()


def test_table_rows_sum_argument_checks(be):
    rng = np.random.RandomState(6)
    keys = _run_keys(rng, (3, 2), 1)
    n = len(keys)
    d_keys = _put_keys(be, keys)
    plan, _ = _build_plan(be, d_keys, n, SUM_ROW_BITS, SUM_ROW_BITS + 5, rng, keys)
    d_rows = _at(be, rng.randn(n * 1028 + 4).astype(np.float32))          # (wide enough for every dim tried)
    d_rows4 = d_rows[1:]
    tables = [rng.randn(r * 16 + 4).astype(np.float32) for r in SUM_ROWS]
    d_tab0, d_tab1 = _at(be, tables[0]), _at(be, tables[1])
    d_tab1_4 = d_tab1[1:]
    for dim in (6, 12, 1028, 0):            # dim % 4; 256 % (dim / 4): 3 lanes a row do not tile a workgroup; dim > 1024
        assert _sum_call(be, plan, n, d_rows, dim, [d_tab0, d_tab1], 1) == UNSUPPORTED, 'dim %d' % dim
    assert _sum_call(be, plan, n, d_rows4, 16, [d_tab0, d_tab1], 1) == UNSUPPORTED
    assert _sum_call(be, plan, 0, d_rows, 16, [d_tab0, d_tab1], 1) == INVALID
    assert _sum_call(be, plan, n, d_rows, 16, [d_tab0, d_tab1], 1, num_modes=0) == INVALID
    assert _sum_call(be, plan, n, d_rows, 16, [d_tab0] * (STEP_MAX_MODES + 1), 1) == INVALID
    assert _sum_call(be, plan, n, d_rows, 16, [d_tab0, d_tab1_4], 1) == INVALID
    assert _sum_call(be, None, n, d_rows, 16, [d_tab0, d_tab1], 1) == INVALID
    assert _sum_call(be, plan, n, None, 16, [d_tab0, d_tab1], 1) == INVALID
    assert be.lib.mpqe_table_rows_sum(be.ptr(plan), n, be.ptr(d_rows), 16, None, 2, 1, be.stream) == INVALID
    np.testing.assert_array_equal(_bits(be, d_tab0), tables[0].view(np.uint32))
    np.testing.assert_array_equal(_bits(be, d_tab1), tables[1].view(np.uint32))


def test_rows_plan_build_argument_checks(be):
    rng = np.random.RandomState(7)
    n, row_bits, key_bits = 40, 4, 9
    keys = rng.randint(0, 2 ** key_bits - 1, size=n).astype(np.uint64)
    d_keys = _put_keys(be, keys)
    pb, wb = be.lib.mpqe_rows_plan_bytes(n), be.lib.mpqe_rows_plan_workspace_bytes(n, key_bits)
    plan, ws = _garbage(be, rng, pb), _garbage(be, rng, wb)
    before = _bits(be, plan)
    plan16, ws16 = plan[4:], ws[4:]                                   # 16 bytes past the boundary

    def call(keys=d_keys, n=n, row_bits=row_bits, key_bits=key_bits, plan=plan, pb=pb, ws=ws, wb=wb):
        return be.lib.mpqe_rows_plan_build(be.ptr(keys), n, row_bits, key_bits, be.ptr(plan), pb, be.ptr(ws), wb, be.stream)
    assert be.lib.mpqe_rows_plan_bytes(0) == 0 and be.lib.mpqe_rows_plan_workspace_bytes(n, 65) == 0
    assert call(key_bits=row_bits) == INVALID
    assert call(key_bits=row_bits - 1) == INVALID
    assert call(key_bits=65) == INVALID
    assert call(row_bits=0) == INVALID
    assert call(n=0) == INVALID
    assert call(keys=None) == INVALID
    assert call(plan=None) == INVALID
    assert call(ws=None) == INVALID
    assert call(pb=pb - 1) == WORKSPACE
    assert call(wb=wb - 1) == WORKSPACE
    assert call(plan=plan16) == INVALID
    assert call(ws=ws16) == INVALID
    np.testing.assert_array_equal(_bits(be, plan), before)
    assert call() == OK
    M, rb, kb, _, skeys, perm = _read_plan(np.ascontiguousarray(be.get(plan)).view(np.uint8), n)
    assert (M, rb, kb) == (n, row_bits, key_bits)
    np.testing.assert_array_equal(perm, np.argsort(keys, kind='stable').astype(np.int32))
    np.testing.assert_array_equal(skeys, np.sort(keys))
