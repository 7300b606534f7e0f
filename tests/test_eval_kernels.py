"""csrc/eval.hip through the C ABI (mpqe_eval_counts, mpqe_eval_auc), on the host emulator and (gpu) on the real library.
Every comparison is exact: the counts against Python ints and evaluation.percentile_of_score, the AUC statistic against a
Python-int double loop and evaluation.roc_auc -- to the bit, since both kernels do integer work only.

Operand hygiene is tests/test_kg_kernels.py's (its helpers are used): outputs sit between guard words that must keep their
bits, outputs and workspace start as garbage, int64 operands start 8 bytes past a 16-byte boundary and fp32 operands 4
bytes past one, and the workspace is exactly as large as mpqe_eval_auc_workspace_bytes says (it lies between guards too)."""
import numpy as np
import pytest
import torch

from mpqe_amd import _capi, evaluation, ops
from tests import test_kg_kernels as K

be = K.be
BAD_INDEX = _capi.FLAG_BAD_INDEX
OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
RS_TILE = 2048              # csrc/radix_sort.h: items of one workgroup of the sort
EV_LONG = 512               # csrc/eval.hip: lists longer than this are counted by a workgroup (rounds of 256), not a wave
FIVE = np.array([-1.5, -0.25, 0.0, 0.5, 2.0], dtype=np.float32)
LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257]
NAN, INF = np.float32(np.nan), np.float32(np.inf)


# ------------------------------------------------------------------------------------------------------ counts
def _counts(be, scores, offsets, B, total, rng):
    """one mpqe_eval_counts call -> (counts [2, B] as the call left them, their bits before it, the error word)"""
    d_scores, d_off = K._at(be, scores, 4), K._at(be, offsets, 8)
    err = be.zeros((1,), np.int32)
    buf, view, before = K._fenced(be, rng, 2 * B, item=8)
    be.check(be.lib.mpqe_eval_counts(be.ptr(d_scores), be.ptr(d_off), B, total, be.ptr(view), be.ptr(err), be.stream),
             'mpqe_eval_counts')
    K._guards_kept(be, buf, before, 2 * B, 'counts')
    np.testing.assert_array_equal(be.get(d_scores).view(np.int32), scores.view(np.int32), err_msg='scores were written')
    return (be.get(view).reshape(2, B).copy(), before[K.GUARD:K.GUARD + 2 * B].reshape(2, B).copy(),
            int(be.get(err)[0]))


def _oracle_counts(scores, lo, hi, B, i):
    t = float(scores[i])
    seg = [float(s) for s in scores[B + lo:B + hi]]
    return sum(1 for s in seg if s < t), sum(1 for s in seg if s <= t)


def _lengths(B):
    if B == 1:
        return [3000]
    if B == 3:
        return [0, 3000, 65]
    lens = (LENGTHS * 6)[:B]
    if B == 65:                 # the threshold between the two kernels from both sides, and twenty rounds of a workgroup
        lens[13], lens[26], lens[40] = EV_LONG, EV_LONG + 1, 5000
    return lens


def _plant(scores, off, B, rng):
    """the special cases, each on a query whose list is long enough; -> the queries whose percentile involves a NaN target
    (none: NaN compares false, the percentile is 0.0 and finite)"""
    lens = np.diff(off)
    have = [i for i in range(B) if lens[i] >= 2]
    neg = scores[B:]

    def seg(i):
        return neg[off[i]:off[i + 1]]
    if len(have) >= 6:
        a, b, c, d, e, f = have[:6]
        scores[a] = np.float32(0.1)
        seg(a)[lens[a] // 2] = scores[a]                # a negative that IS the target: bit-equal, ties
        scores[b] = NAN                                 # a NaN target: below nothing, equal to nothing
        seg(c)[::2] = NAN                               # NaN negatives: never counted
        seg(d)[0], seg(d)[-1] = INF, -INF
        scores[e] = INF                                 # +inf target ties with +inf negatives
        seg(e)[0], seg(e)[1] = INF, -INF
        scores[f] = np.float32(-0.0)                    # -0.0 == +0.0 (FIVE holds +0.0)
        seg(f)[0] = np.float32(0.0)
    else:                                               # B = 1, 3: the long list gets them all
        i = int(np.argmax(lens))
        scores[i] = np.float32(-0.0)
        seg(i)[:6] = [0.0, -0.0, NAN, INF, -INF, 0.5]


@pytest.mark.parametrize('B', [1, 3, 64, 65])
def test_counts_match_python_ints_and_percentile_of_score(be, B):
    rng = np.random.RandomState(100 + B)
    lens = np.array(_lengths(B), dtype=np.int64)
    off = np.zeros(B + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    total = int(off[-1])
    scores = FIVE[rng.randint(0, 5, size=B + total)]    # five distinct values: ties dominate
    _plant(scores, off, B, rng)
    got, _, flags = _counts(be, scores, off, B, total, rng)
    assert flags == 0
    want = np.array([_oracle_counts(scores, off[i], off[i + 1], B, i) for i in range(B)], dtype=np.int64).T
    np.testing.assert_array_equal(got, want)
    # the percentile from the two counts, as ops.eval_percentiles forms it on the device, is percentile_of_score's to the bit
    perc = ops.eval_percentiles(torch.from_numpy(got), torch.from_numpy(off)).numpy()
    ref = np.array([evaluation.percentile_of_score(scores[B + off[i]:B + off[i + 1]], scores[i]) for i in range(B)],
                   dtype=np.float64)
    assert perc.dtype == np.float64
    np.testing.assert_array_equal(np.isnan(perc), lens == 0)             # n = 0 -> NaN, nothing else is
    np.testing.assert_array_equal(perc[lens > 0].view(np.int64), ref[lens > 0].view(np.int64))
    # the mean of a NaN-free set: a reordered float64 sum of Q non-negative terms is within Q 2^-52 relative of np.mean's
    keep = torch.from_numpy(np.nonzero(lens > 0)[0])
    Q = int(keep.shape[0])
    mean = float(torch.from_numpy(perc)[keep].mean())
    assert abs(mean - np.mean(ref[lens > 0])) <= Q * 2.0 ** -52 * np.mean(ref[lens > 0])


@pytest.mark.parametrize('case', ['decreasing', 'past_total', 'negative'])
def test_counts_with_corrupt_offsets_flag_and_skip_only_those_queries(be, case):
    rng = np.random.RandomState(7)
    B = 6
    off = np.array([0, 3, 7, 607, 612, 614, 1314], dtype=np.int64)      # lists of 3, 4, 600, 5, 2, 700 scores
    total = 1314
    scores = FIVE[rng.randint(0, 5, size=B + total)]
    if case == 'decreasing':
        off[4] = 600            # query 3 runs backwards [607, 600); query 4 is [600, 614): in order and inside, so counted
        bad = [3]
    elif case == 'past_total':
        off[6] = total + 5      # the long list of query 5 ends past the scores
        bad = [5]
    else:
        off[0] = -1
        bad = [0]
    got, before, flags = _counts(be, scores, off, B, total, rng)
    assert flags == BAD_INDEX
    for i in range(B):
        if i in bad:
            np.testing.assert_array_equal(got[:, i], before[:, i], err_msg='query %d was written' % i)
        else:
            assert tuple(got[:, i]) == _oracle_counts(scores, off[i], off[i + 1], B, i), i


def test_counts_argument_checks(be):
    s, o = be.zeros((4,), np.float32), be.zeros((2,), np.int64)
    out = be.zeros((2,), np.int64)
    lib = be.lib
    assert lib.mpqe_eval_counts(be.ptr(s), be.ptr(o), -1, 3, be.ptr(out), None, be.stream) == INVALID
    assert lib.mpqe_eval_counts(be.ptr(s), be.ptr(o), 1, -1, be.ptr(out), None, be.stream) == INVALID
    assert lib.mpqe_eval_counts(None, be.ptr(o), 1, 3, be.ptr(out), None, be.stream) == INVALID
    assert lib.mpqe_eval_counts(be.ptr(s), be.ptr(o), 1, 2 ** 31, be.ptr(out), None, be.stream) == UNSUPPORTED
    assert lib.mpqe_eval_counts(None, None, 0, 0, None, None, be.stream) == OK


# --------------------------------------------------------------------------------------------------------- AUC
def _auc(be, pos, neg, rng, n_pos=None, short=0):
    """one mpqe_eval_auc call, the workspace exactly as large as declared and fenced -> (status, U2 or None when the call
    was refused -- the output word and the workspace then kept their bits)"""
    n_pos = len(pos) if n_pos is None else n_pos
    d_pos, d_neg = K._at(be, pos, 4), K._at(be, neg, 4)
    need = be.lib.mpqe_eval_auc_workspace_bytes(max(n_pos, 1), len(neg))
    assert need > 0 and need % 4 == 0
    w_buf, w_view, w_before = K._fenced(be, rng, need // 4)
    o_buf, o_view, o_before = K._fenced(be, rng, 1, item=8)
    st = be.lib.mpqe_eval_auc(be.ptr(d_pos), n_pos, be.ptr(d_neg), len(neg), be.ptr(o_view), be.ptr(w_view), need - short,
                              be.stream)
    K._guards_kept(be, w_buf, w_before, need // 4, 'the workspace')
    K._guards_kept(be, o_buf, o_before, 1, 'U2')
    np.testing.assert_array_equal(be.get(d_pos).view(np.int32), pos.view(np.int32), err_msg='pos was written')
    np.testing.assert_array_equal(be.get(d_neg).view(np.int32), neg.view(np.int32), err_msg='neg was written')
    if st != OK:
        np.testing.assert_array_equal(be.get(w_buf), w_before, err_msg='a refused call wrote its workspace')
        np.testing.assert_array_equal(be.get(o_buf), o_before, err_msg='a refused call wrote its output')
        return st, None
    return st, int(be.get(o_view).view(np.uint64)[0])


def _canon(x):
    x = float(x)
    return 0.0 if x != x else x                         # np.nan_to_num; -0.0 == 0.0 and +-inf are Python's already


def _brute(pos, neg):
    u2 = 0
    cn = [_canon(x) for x in neg]
    for p in pos:
        p = _canon(p)
        for x in cn:
            u2 += 2 if x < p else (1 if x == p else 0)
    return u2


def _host_auc(pos, neg):
    """the list path: roc_auc over np.nan_to_num of the scores as Python floats (evaluation.eval_auc_queries)"""
    scores = np.nan_to_num(np.asarray(pos.tolist() + neg.tolist(), dtype=np.float64))
    return evaluation.roc_auc([1] * len(pos) + [0] * len(neg), scores)


def _scores(kind, n, rng):
    if kind == 'random':
        return rng.randn(n).astype(np.float32)
    s = FIVE[rng.randint(0, 5, size=n)]
    if kind == 'mixed':         # NaN (ranks as 0.0, which FIVE holds), +-inf, both zeros, and a few values of their own
        special = np.array([NAN, INF, -INF, 0.0, -0.0, 1e-42, -1e-42, 3.4e38], dtype=np.float32)
        pick = rng.rand(n) < 0.4
        s[pick] = special[rng.randint(0, len(special), size=int(pick.sum()))]
        s[rng.rand(n) < 0.1] = np.float32(rng.randn())
    return s


SHAPES = [(3, 1), (1, 2), (70, RS_TILE - 1), (300, RS_TILE), (RS_TILE + 5, RS_TILE + 1), (257, 3 * RS_TILE + 7)]


@pytest.mark.parametrize('kind', ['ties', 'mixed', 'random'])
@pytest.mark.parametrize('n_pos,n_neg', SHAPES)
def test_auc_statistic_is_exact_and_equals_roc_auc(be, n_pos, n_neg, kind):
    rng = np.random.RandomState(n_pos * 7 + n_neg)
    pos, neg = _scores(kind, n_pos, rng), _scores(kind, n_neg, rng)
    if kind == 'mixed' and n_neg >= 2:
        neg[0], neg[1] = NAN, np.float32(-0.0)          # (whatever the draw: NaN, -0.0 and +0.0 must tie)
        pos[0] = np.float32(0.0)
    st, u2 = _auc(be, pos, neg, rng)
    assert st == OK
    if n_pos * n_neg <= 700000:
        assert u2 == _brute(pos, neg)
    assert 0 <= u2 <= 2 * n_pos * n_neg
    want = _host_auc(pos, neg)
    got = np.float64(ops.auc_from_statistic(u2, n_pos, n_neg))
    assert got.view(np.int64) == np.float64(want).view(np.int64), (got, want)
    st, again = _auc(be, pos, neg, rng)                 # other garbage in workspace and output: the same bits
    assert st == OK and again == u2


@pytest.mark.parametrize('n_pos,n_neg', [(5, 3), (130, RS_TILE + 1)])
def test_auc_extremes(be, n_pos, n_neg):
    rng = np.random.RandomState(3)
    same = np.full(n_pos, 0.25, dtype=np.float32), np.full(n_neg, 0.25, dtype=np.float32)
    st, u2 = _auc(be, same[0], same[1], rng)
    assert st == OK and u2 == n_pos * n_neg and ops.auc_from_statistic(u2, n_pos, n_neg) == 0.5
    lo, hi = FIVE[rng.randint(0, 2, size=n_neg)], FIVE[rng.randint(3, 5, size=n_pos)]
    st, u2 = _auc(be, hi, lo, rng)                      # every positive above every negative
    assert st == OK and ops.auc_from_statistic(u2, n_pos, n_neg) == 1.0
    st, u2 = _auc(be, lo, hi, rng)                      # every positive below
    assert st == OK and u2 == 0


def test_auc_refusals_write_nothing(be):
    rng = np.random.RandomState(4)
    pos, neg = _scores('ties', 40, rng), _scores('ties', RS_TILE + 9, rng)
    assert _auc(be, pos, neg, rng, short=1) == (WORKSPACE, None)
    assert _auc(be, pos, neg, rng, n_pos=0) == (INVALID, None)
    lib = be.lib
    d = be.zeros((4,), np.float32)
    out = be.zeros((1,), np.int64)
    ws = be.zeros((4096,), np.int32)
    assert lib.mpqe_eval_auc(be.ptr(d), 4, be.ptr(d), 0, be.ptr(out), be.ptr(ws), 16384, be.stream) == INVALID
    assert lib.mpqe_eval_auc(be.ptr(d), 2 ** 31, be.ptr(d), 4, be.ptr(out), be.ptr(ws), 16384, be.stream) == UNSUPPORTED
    assert lib.mpqe_eval_auc(be.ptr(d), 4, be.ptr(d), 4, be.ptr(out), be.ptr(ws) + 2, 16000, be.stream) == INVALID
    assert lib.mpqe_eval_auc_workspace_bytes(0, 4) == 0 and lib.mpqe_eval_auc_workspace_bytes(4, 2 ** 31) == 0
    assert int(be.get(out)[0]) == 0


def test_ops_wrappers_on_the_emulator():
    """ops.eval_counts / ops.eval_auc with lib= (CPU tensors on the host emulator): shapes, the error word, the ValueError"""
    from tests.kernel_backend import EmuBackend
    lib = EmuBackend().lib
    scores = torch.tensor([0.5, 0.0, 0.5, 0.25, 1.0, -1.0], dtype=torch.float32)
    off = torch.tensor([0, 3, 4], dtype=torch.int64)
    counts = ops.eval_counts(scores, off, 2, lib=lib)
    assert counts.tolist() == [[1, 1], [2, 1]]
    assert ops.eval_percentiles(counts, off).tolist() == [200.0 / 3, 100.0]
    with pytest.raises(IndexError):
        ops.eval_counts(scores, torch.tensor([0, 5, 4], dtype=torch.int64), 2, lib=lib)
    assert ops.eval_auc(scores[:2], scores[2:], lib=lib) == (2 * 2 + 1) + 2 * 1      # 0.5: two below, one tie; 0.0: one below
    with pytest.raises(ValueError, match='Only one class present'):
        ops.eval_auc(scores[:0], scores, lib=lib)
