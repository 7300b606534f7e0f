"""mpqe_eval_auc_segments (csrc/eval.hip) through the C ABI, on the host emulator and (gpu) on the real library: the
ROC-AUC statistic of S slices in one call. Every comparison is exact -- the kernel does integer work only: against Python
ints (a double loop where it is small, sorted searches on float64 otherwise) and against mpqe_eval_auc on every slice
alone, on the same backend.

Operands sit between fences (tests/fenced.py): fp32 operands 4 bytes past a 16-byte boundary, the workspace exactly as
large as mpqe_eval_auc_segments_workspace_bytes says, the output between integer fences."""
import numpy as np
import pytest
import torch

from mpqe_amd import ops
from tests.fenced import assert_fence_intact, fenced, fenced_bytes
from tests.test_gqe_kernels import INVALID, OK, UNSUPPORTED, WORKSPACE, be  # noqa: F401  (`be`: the backend fixture)

RS_TILE = 2048              # csrc/radix_sort.h: items of one workgroup of the sort
FIVE = np.array([-1.5, -0.25, 0.0, 0.5, 2.0], dtype=np.float32)
NAN, INF = np.float32(np.nan), np.float32(np.inf)
SIZES = [0, 1, 63, 64, 65, RS_TILE, RS_TILE + 1]


def _canon(x):
    x = np.nan_to_num(np.asarray(x, dtype=np.float64), nan=0.0, posinf=np.inf, neginf=-np.inf)
    return x + 0.0                                      # (-0.0 + 0.0 = +0.0)


def _exact(pos, neg):
    """U2 as a Python int: per positive 2 |{neg < p}| + |{neg == p}| by two searches in the sorted float64 negatives"""
    cn = np.sort(_canon(neg))
    cp = _canon(pos)
    lo, hi = np.searchsorted(cn, cp, side='left'), np.searchsorted(cn, cp, side='right')
    return int(lo.sum()) + int(hi.sum())


def _brute(pos, neg):
    u2 = 0
    cn = [float(x) for x in _canon(neg)]
    for p in _canon(pos):
        p = float(p)
        for x in cn:
            u2 += 2 if x < p else (1 if x == p else 0)
    return u2


def _scores(kind, n, rng):
    if kind == 'random':
        return rng.randn(n).astype(np.float32)
    s = FIVE[rng.randint(0, 5, size=n)]
    if kind == 'mixed':         # NaN (ranks as 0.0, which FIVE holds), +-inf, both zeros, and a few values of their own
        special = np.array([NAN, INF, -INF, 0.0, -0.0, 1e-42, -1e-42, 3.4e38], dtype=np.float32)
        pick = rng.rand(n) < 0.4
        s[pick] = special[rng.randint(0, len(special), size=int(pick.sum()))]
    return s


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _place(be, a, **kw):
    """fenced(); an empty operand (whose view would forget its address) is a plain empty array"""
    return fenced(be, a, **kw) if a.size else be.put(a)


def _segments(be, pos, neg, pos_off, neg_off, fill='noise', short=0):
    """one call -> (status, u2 as Python ints, or None for a refused call -- which wrote nothing)"""
    S = len(pos_off) - 1
    d_pos, d_neg = _place(be, pos, misalign=1), _place(be, neg, misalign=1)
    d_po, d_no = fenced(be, pos_off), fenced(be, neg_off)
    need = be.lib.mpqe_eval_auc_segments_workspace_bytes(len(pos), len(neg), S)
    assert need > 0
    ws = fenced_bytes(be, need - short, fill, align=8)
    before = be.get(ws).copy()
    out = fenced(be, np.full(S, -5, dtype=np.int64))
    st = be.lib.mpqe_eval_auc_segments(be.ptr(d_pos), len(pos), be.ptr(d_neg), len(neg), be.ptr(d_po), be.ptr(d_no), S,
                                       be.ptr(out), be.ptr(ws), need - short, be.stream)
    got = be.get(out)
    for view, what in ((ws, 'the workspace'), (out, 'u2'), (d_pos, 'pos'), (d_neg, 'neg'), (d_po, 'pos_off'),
                       (d_no, 'neg_off')):
        if int(view.shape[0]):
            assert_fence_intact(be, view, what)
    np.testing.assert_array_equal(be.get(d_pos).view(np.int32), pos.view(np.int32), err_msg='pos was written')
    np.testing.assert_array_equal(be.get(d_neg).view(np.int32), neg.view(np.int32), err_msg='neg was written')
    if st != OK:
        np.testing.assert_array_equal(be.get(ws), before, err_msg='a refused call wrote its workspace')
        assert (got == -5).all(), 'a refused call wrote its output'
        return st, None
    return st, [int(v) for v in got.view(np.uint64)]


def _single(be, pos, neg):
    """mpqe_eval_auc on one slice"""
    need = be.lib.mpqe_eval_auc_workspace_bytes(len(pos), len(neg))
    ws = be.nbytes(need)
    out = be.zeros((1,), np.int64)
    d_pos, d_neg = be.put(pos), be.put(neg)
    assert be.lib.mpqe_eval_auc(be.ptr(d_pos), len(pos), be.ptr(d_neg), len(neg), be.ptr(out), be.ptr(ws), need,
                                be.stream) == OK
    return int(be.get(out).view(np.uint64)[0])


def _check(be, pos, neg, pos_lens, neg_lens, fill='noise', singles=True):
    po, no = _offsets(pos_lens), _offsets(neg_lens)
    st, got = _segments(be, pos, neg, po, no, fill)
    assert st == OK
    for s in range(len(pos_lens)):
        p, n = pos[po[s]:po[s + 1]], neg[no[s]:no[s + 1]]
        want = _exact(p, n)
        assert got[s] == want, (s, len(p), len(n), got[s], want)
        if len(p) * len(n) <= 20000:
            assert want == _brute(p, n)
        if singles and len(p) and len(n):
            assert got[s] == _single(be, p, n), s
        if not len(p) or not len(n):
            assert got[s] == 0
    return got


@pytest.mark.parametrize('kind', ['ties', 'mixed', 'random'])
def test_segment_sizes_with_unequal_sides(be, kind):
    """segments of 0, 1, 63, 64, 65, 2048 and 2049 positives against 64, 65, 2048, 2049, 0, 1, 63 negatives"""
    rng = np.random.RandomState(17 + len(kind))
    pos_lens, neg_lens = SIZES, SIZES[3:] + SIZES[:3]
    pos, neg = _scores(kind, sum(pos_lens), rng), _scores(kind, sum(neg_lens), rng)
    if kind == 'mixed':
        no = _offsets(neg_lens)
        po = _offsets(pos_lens)
        neg[no[2]], neg[no[2] + 1], pos[po[2]] = NAN, np.float32(-0.0), np.float32(0.0)     # NaN, -0.0 and +0.0 tie
        neg[no[3]], pos[po[3]], pos[po[3] + 1] = INF, INF, -INF
    got = _check(be, pos, neg, pos_lens, neg_lens)
    assert got[0] == 0 and got[4] == 0 and sum(got) > 0


@pytest.mark.parametrize('n_pos,n_neg', [(1, 1), (65, RS_TILE + 1), (RS_TILE + 1, 3)])
def test_one_segment_equals_eval_auc(be, n_pos, n_neg):
    rng = np.random.RandomState(n_pos + n_neg)
    pos, neg = _scores('mixed', n_pos, rng), _scores('mixed', n_neg, rng)
    _check(be, pos, neg, [n_pos], [n_neg])


def test_a_thousand_singletons(be):
    rng = np.random.RandomState(5)
    S = 1000
    pos, neg = _scores('ties', S, rng), _scores('ties', S, rng)
    got = _check(be, pos, neg, [1] * S, [1] * S, singles=False)
    assert set(got) == {0, 1, 2}
    for s in (0, 1, 499, 999):
        assert got[s] == _single(be, pos[s:s + 1], neg[s:s + 1])


def test_equal_scores_across_a_boundary_are_not_counted(be):
    """every score the same: u2[s] = n_pos[s] * n_neg[s] (one per pair), whatever the neighbours hold"""
    pos_lens, neg_lens = [3, 1, 0, 70, 2], [1, 65, 4, 2, 300]
    pos = np.full(sum(pos_lens), 0.25, dtype=np.float32)
    neg = np.full(sum(neg_lens), 0.25, dtype=np.float32)
    got = _check(be, pos, neg, pos_lens, neg_lens)
    assert got == [a * b for a, b in zip(pos_lens, neg_lens)]
    # a positive that ties with its own segment's negative and is above / below the neighbours' equal scores
    pos = np.array([1.0, 1.0, 1.0], dtype=np.float32)
    neg = np.array([1.0, 0.5, 1.0, 1.0, 2.0], dtype=np.float32)
    assert _check(be, pos, neg, [1, 1, 1], [1, 2, 2]) == [1, 3, 1]


@pytest.mark.parametrize('fill', ['zeros', 'nan', 'ones', 'one_f32', 'noise'])
def test_workspace_is_exactly_its_declared_size(be, fill):
    rng = np.random.RandomState(9)
    pos_lens, neg_lens = [5, 0, 70, 3], [RS_TILE + 3, 7, 0, 65]
    pos, neg = _scores('mixed', sum(pos_lens), rng), _scores('mixed', sum(neg_lens), rng)
    first = _check(be, pos, neg, pos_lens, neg_lens, fill=fill, singles=False)
    assert first == _check(be, pos, neg, pos_lens, neg_lens, fill='noise', singles=False)
    assert _segments(be, pos, neg, _offsets(pos_lens), _offsets(neg_lens), fill, short=1) == (WORKSPACE, None)


def test_empty_sides_and_refusals(be):
    empty = np.zeros(0, dtype=np.float32)
    some = FIVE.copy()
    off0, off5 = np.array([0, 0, 0], dtype=np.int64), np.array([0, 2, 5], dtype=np.int64)
    assert _segments(be, empty, some, off0, off5) == (OK, [0, 0])
    assert _segments(be, some, empty, off5, off0) == (OK, [0, 0])
    assert _segments(be, empty, empty, off0, off0) == (OK, [0, 0])
    lib = be.lib
    d = be.zeros((8,), np.float32)
    o = be.put(off5)
    out = be.zeros((2,), np.int64)
    ws = be.nbytes(1 << 16)
    assert lib.mpqe_eval_auc_segments(be.ptr(d), 5, be.ptr(d), 5, be.ptr(o), be.ptr(o), 0, be.ptr(out), be.ptr(ws), 1 << 16,
                                      be.stream) == INVALID
    assert lib.mpqe_eval_auc_segments(be.ptr(d), 5, be.ptr(d), 5, None, be.ptr(o), 2, be.ptr(out), be.ptr(ws), 1 << 16,
                                      be.stream) == INVALID
    assert lib.mpqe_eval_auc_segments(be.ptr(d), 2 ** 31, be.ptr(d), 5, be.ptr(o), be.ptr(o), 2, be.ptr(out), be.ptr(ws),
                                      1 << 16, be.stream) == UNSUPPORTED
    assert lib.mpqe_eval_auc_segments_workspace_bytes(5, 5, 0) == 0
    assert lib.mpqe_eval_auc_segments_workspace_bytes(5, 2 ** 31, 2) == 0
    assert int(be.get(out)[0]) == 0


def test_corrupt_offsets_stay_inside_the_arrays(be):
    """offsets out of order or past the end: the call returns, the fences hold (nothing is read or written outside the
    operands), and the segments whose offsets are in order and inside keep their exact statistic"""
    rng = np.random.RandomState(11)
    pos, neg = _scores('ties', 40, rng), _scores('ties', 90, rng)
    po = np.array([0, 10, 20, 30, 40], dtype=np.int64)
    no = np.array([0, 30, 20, 60, 90], dtype=np.int64)          # segment 1 runs backwards
    st, got = _segments(be, pos, neg, po, no)
    assert st == OK and got[1] == 0
    no = np.array([0, 30, 50, 60, 95], dtype=np.int64)          # the last one ends past the negatives
    st, got = _segments(be, pos, neg, po, no)
    assert st == OK and got[3] == 0
    assert got[0] == _exact(pos[:10], neg[:30]) and got[1] == _exact(pos[10:20], neg[30:50])


def test_ops_wrapper_on_the_emulator():
    from tests.kernel_backend import EmuBackend
    lib = EmuBackend().lib
    pos = torch.tensor([0.5, 0.0, 0.5], dtype=torch.float32)
    neg = torch.tensor([0.5, 0.25, 1.0, -1.0, 0.5], dtype=torch.float32)
    po, no = torch.tensor([0, 2, 2, 3]), torch.tensor([0, 4, 5, 5])
    u2 = ops.eval_auc_segments(pos, neg, po, no, lib=lib)
    assert u2.dtype == torch.int64 and u2.tolist() == [ops.eval_auc(pos[:2], neg[:4], lib=lib), 0, 0]
    assert ops.auc_from_statistic(int(u2[0]), 2, 4) == ops.eval_auc(pos[:2], neg[:4], lib=lib) / 16
    with pytest.raises(ValueError):
        ops.eval_auc_segments(pos, neg, po, no[:3], lib=lib)
