"""The guarded parameter updates of the C ABI (include/mpqe_amd.h: mpqe_adam_step_guarded, mpqe_sgd_step_guarded,
mpqe_adam_rows_step_guarded): with the guard word at 0 they write the bits of the unguarded entry points and count the
update once; with the word set they write nothing at all. On the host emulator and (gpu) on the real library. The word is
only ever set from the host here."""
import ctypes

import numpy as np
import pytest

OK, INVALID, UNSUPPORTED = 0, -1, -2
FLAGGED = (1, 16 | 0x200, 32)          # a bad entity id; a timed-out hand-off with its site; an unbuilt touch plan
HYPER = (0.01, 0.9, 0.999, 1e-8, 1e-2)  # lr, beta1, beta2, eps, weight decay


@pytest.fixture(scope='module', params=['emu', pytest.param('hip', marks=pytest.mark.gpu)])
def be(request):
    from tests import kernel_backend
    return kernel_backend.EmuBackend() if request.param == 'emu' else kernel_backend.HipBackend()


def _bits(be, a):
    return np.ascontiguousarray(be.get(a)).view(np.uint32).copy()


def _buffers(be, rng, n, offset):
    """p, g, m, v [n] on the backend; offset = 1: every buffer starts 4 bytes past its 16-byte boundary (the kernels'
    scalar path). Views of the allocations, so the pointers carry the offset."""
    host = [rng.randn(n + offset).astype(np.float32) for _ in range(4)]
    host[3] = np.abs(host[3])                        # second moment
    return [be.put(h)[offset:] for h in host]


def _dense_call(be, kind, guarded, bufs, n, step, word=None, applied=None, hyper=HYPER):
    p, g, m, v = [be.ptr(x) for x in bufs]
    lr, b1, b2, eps, wd = hyper
    if kind == 'adam':
        args = (p, g, m, v, n, lr, b1, b2, eps, wd, step)
        name = 'mpqe_adam_step'
    else:
        args = (p, g, n, lr, wd)
        name = 'mpqe_sgd_step'
    if guarded:
        return getattr(be.lib, name + '_guarded')(*(args + (be.ptr(word), be.ptr(applied), be.stream)))
    return getattr(be.lib, name)(*(args + (be.stream,)))


def _check_dense(be, kind, n, offset, seed=0):
    rng = np.random.RandomState(seed + n)
    ref = _buffers(be, rng, n, offset)
    rng = np.random.RandomState(seed + n)
    got = _buffers(be, rng, n, offset)
    state = [0, 2, 3] if kind == 'adam' else [0]       # p, m, v (the gradient is read only)
    word, applied = be.zeros(1, np.int32), be.zeros(1, np.int64)
    # step 1, clean word: the unguarded entry point's bits, counted once
    assert _dense_call(be, kind, False, ref, n, 1) == OK
    assert _dense_call(be, kind, True, got, n, 1, word, applied) == OK
    for i in state:
        np.testing.assert_array_equal(_bits(be, got[i]), _bits(be, ref[i]), err_msg='step 1, buffer %d' % i)
    assert int(be.get(applied)[0]) == 1
    # the word set: nothing is written, nothing counted, and the call itself succeeds
    before = [_bits(be, got[i]) for i in range(4)]
    for flags in FLAGGED:
        word[0] = flags
        assert _dense_call(be, kind, True, got, n, 2, word, applied) == OK
        for i in range(4):
            np.testing.assert_array_equal(_bits(be, got[i]), before[i], err_msg='word %#x, buffer %d' % (flags, i))
        assert int(be.get(applied)[0]) == 1
        assert int(be.get(word)[0]) == flags           # (the update reads the word, it never clears it)
    # cleared again: the next call applies, the counter advances by one
    word[0] = 0
    assert _dense_call(be, kind, False, ref, n, 2) == OK
    assert _dense_call(be, kind, True, got, n, 2, word, applied) == OK
    for i in state:
        np.testing.assert_array_equal(_bits(be, got[i]), _bits(be, ref[i]), err_msg='step 2, buffer %d' % i)
    assert int(be.get(applied)[0]) == 2
    np.testing.assert_array_equal(_bits(be, got[1]), before[1])      # the gradient buffer is never written


@pytest.mark.parametrize('offset', [0, 1], ids=['aligned', 'plus4bytes'])
@pytest.mark.parametrize('n', [1, 3, 4, 5, 1023, 4 * 1024 + 1])
@pytest.mark.parametrize('kind', ['adam', 'sgd'])
def test_dense_guarded_update(be, kind, n, offset):
    _check_dense(be, kind, n, offset)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['adam', 'sgd'])
def test_dense_guarded_update_beyond_the_grid_cap(kind):
    """n = 4 * 2^20 + 7: more than 4096 workgroups' worth even at four elements a thread, so the grid-stride loop takes a
    second trip -- and still one thread of the launch counts the update."""
    from tests import kernel_backend
    _check_dense(kernel_backend.HipBackend(), kind, 4 * 2 ** 20 + 7, 0)


def test_dense_guarded_update_without_a_counter(be):
    """applied = NULL is accepted: the update happens (or is refused) all the same."""
    n = 77
    for kind in ('adam', 'sgd'):
        ref = _buffers(be, np.random.RandomState(3), n, 0)
        got = _buffers(be, np.random.RandomState(3), n, 0)
        word = be.zeros(1, np.int32)
        assert _dense_call(be, kind, False, ref, n, 1) == OK
        assert _dense_call(be, kind, True, got, n, 1, word, None) == OK
        np.testing.assert_array_equal(_bits(be, got[0]), _bits(be, ref[0]))
        word[0] = 1
        assert _dense_call(be, kind, True, got, n, 2, word, None) == OK
        np.testing.assert_array_equal(_bits(be, got[0]), _bits(be, ref[0]))


def test_dense_guarded_argument_checks(be):
    n = 8
    bufs = _buffers(be, np.random.RandomState(1), n, 0)
    word, applied = be.zeros(1, np.int32), be.zeros(1, np.int64)
    before = [_bits(be, b) for b in bufs]
    for kind in ('adam', 'sgd'):
        assert _dense_call(be, kind, True, bufs, n, 1, None, applied) == INVALID          # the guard is required
        assert _dense_call(be, kind, True, bufs, 0, 1, word, applied) == INVALID          # ... and the old checks hold
        assert _dense_call(be, kind, True, [None] + bufs[1:], n, 1, word, applied) == INVALID
        assert _dense_call(be, kind, True, [bufs[0], None] + bufs[2:], n, 1, word, applied) == INVALID
    assert _dense_call(be, 'adam', True, bufs, n, 0, word, applied) == INVALID            # step >= 1
    assert _dense_call(be, 'adam', True, bufs[:2] + [None, bufs[3]], n, 1, word, applied) == INVALID
    assert _dense_call(be, 'adam', True, bufs, n, 1, word, applied, hyper=(0.01, 1.0, 0.999, 1e-8, 0.0)) == INVALID
    for b, want in zip(bufs, before):
        np.testing.assert_array_equal(_bits(be, b), want)
    assert int(be.get(applied)[0]) == 0


# ------------------------------------------------------------------------------------------------ row-sparse Adam
ROWS = (11, 9)          # two tables
ROW_BITS = 4


def _rows_plan(be, rng, n=40):
    """A plan over n (40) (table, row) keys of two tables, keys repeated; returns (buffer, pointer, entries, touched rows)."""
    tab = rng.randint(0, 2, size=n)
    row = np.where(tab == 0, rng.randint(0, 6, size=n), rng.randint(2, 7, size=n))         # rows 6.. / 0,1,7.. stay untouched
    keys = (tab.astype(np.uint64) << np.uint64(ROW_BITS)) | row.astype(np.uint64)
    assert n == 1 or len(np.unique(keys)) < len(keys)
    pb = be.lib.mpqe_rows_plan_bytes(n)
    wb = be.lib.mpqe_rows_plan_workspace_bytes(n, ROW_BITS + 5)
    plan, ws = be.nbytes(pb + 256), be.nbytes(wb + 256)
    pptr = (be.ptr(plan) + 255) // 256 * 256
    d_keys = be.put(keys.view(np.int64))              # (the same 8 bytes: torch has no uint64 arithmetic to offer)
    be.check(be.lib.mpqe_rows_plan_build(be.ptr(d_keys), n, ROW_BITS, ROW_BITS + 5, pptr, pb,
                                         (be.ptr(ws) + 255) // 256 * 256, wb, be.stream), 'rows plan')
    be.get(plan)                                          # (the build has run before its inputs go away)
    touched = [sorted(set(row[tab == t].tolist())) for t in range(2)]
    return plan, pptr, n, touched


def _rows_call(be, guarded, pptr, n, tabs, D, step, word=None, applied=None):
    arr = ctypes.c_void_p * 2
    cols = [arr(*[be.ptr(t[i]) for t in tabs]) for i in range(4)]           # params, grads, exp_avg, exp_avg_sq
    args = (pptr, n, cols[0], cols[1], cols[2], cols[3], 2, D, 0.05, 0.9, 0.99, 1e-6, step)
    if guarded:
        return be.lib.mpqe_adam_rows_step_guarded(*(args + (be.ptr(word), be.ptr(applied), be.stream)))
    return be.lib.mpqe_adam_rows_step(*(args + (be.stream,)))


def _tables(be, D, seed):
    rng = np.random.RandomState(seed)
    out = []
    for r in ROWS:
        host = [rng.randn(r, D).astype(np.float32) for _ in range(4)]
        host[3] = np.abs(host[3])
        out.append([be.put(h) for h in host])
    return out


@pytest.mark.parametrize('D', [16, 128])
def test_rows_guarded_update(be, D, n=40):
    """D = 16: 4 lanes a row, 64 rows a workgroup (one workgroup); D = 128: 32 lanes a row, 8 rows a workgroup (five).
    (n: for tests/test_workspace_bounds.py, which runs this on plans of other sizes; one key touches one table.)"""
    plan, pptr, n, touched = _rows_plan(be, np.random.RandomState(11), n)
    ref, got = _tables(be, D, 21), _tables(be, D, 21)
    start = [[_bits(be, x) for x in t] for t in got]
    word, applied = be.zeros(1, np.int32), be.zeros(1, np.int64)
    # the word set: nothing is written
    for flags in FLAGGED:
        word[0] = flags
        assert _rows_call(be, True, pptr, n, got, D, 1, word, applied) == OK
        for t in range(2):
            for i in range(4):
                np.testing.assert_array_equal(_bits(be, got[t][i]), start[t][i], err_msg='word %#x' % flags)
        assert int(be.get(applied)[0]) == 0
    # clean: the unguarded entry point's bits over two steps, each counted once; untouched rows keep theirs
    word[0] = 0
    for step in (1, 2):
        assert _rows_call(be, False, pptr, n, ref, D, step) == OK
        assert _rows_call(be, True, pptr, n, got, D, step, word, applied) == OK
        for t in range(2):
            for i in range(4):
                np.testing.assert_array_equal(_bits(be, got[t][i]), _bits(be, ref[t][i]), err_msg='step %d' % step)
        assert int(be.get(applied)[0]) == step
    for t in range(2):
        rest = sorted(set(range(ROWS[t])) - set(touched[t]))
        assert rest and (touched[t] or n == 1)
        for i in (0, 2, 3):
            now = _bits(be, got[t][i])
            np.testing.assert_array_equal(now[rest], start[t][i][rest])
            assert (now[touched[t]] != start[t][i][touched[t]]).any(axis=1).all(), 'a touched row was not updated'


def test_rows_guarded_argument_checks(be):
    D = 16
    plan, pptr, n, _ = _rows_plan(be, np.random.RandomState(11))
    tabs = _tables(be, D, 5)
    start = [[_bits(be, x) for x in t] for t in tabs]
    word = be.zeros(1, np.int32)
    assert _rows_call(be, True, pptr, n, tabs, D, 1, None, None) == INVALID           # the guard is required
    assert _rows_call(be, True, None, n, tabs, D, 1, word, None) == INVALID           # ... and the old checks hold
    assert _rows_call(be, True, pptr, 0, tabs, D, 1, word, None) == INVALID
    assert _rows_call(be, True, pptr, n, tabs, D, 0, word, None) == INVALID
    assert _rows_call(be, True, pptr, n, tabs, 6, 1, word, None) == UNSUPPORTED
    for t in range(2):
        for i in range(4):
            np.testing.assert_array_equal(_bits(be, tabs[t][i]), start[t][i])
    # no counter: accepted, and the update happens
    assert _rows_call(be, True, pptr, n, tabs, D, 1, word, None) == OK
    assert (_bits(be, tabs[0][0]) != start[0][0]).any()
