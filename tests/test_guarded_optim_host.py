"""FlatOptimizer's choice of entry points, without a GPU: guard=True calls the guarded entry point for EVERY launch of an
update with the step's error word and hands the applied-update counter to the LAST launch only; guard=False calls the old
entry points with the old arguments. A hand-built step object and a recording stand-in for the library; the host's step
count follows the (here: host-resident) counter once an error word has been cleared. And mpqe_amd.optim.Adam / SGD accept
guard= on the torch fallback."""
import contextlib
import types

import pytest
import torch

from mpqe_amd import ops, optim


class _Recorder(object):
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith('mpqe_'):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


class _Encoder(object):
    def __init__(self, tables):
        self._tables = tables

    def table(self, mode):
        return self._tables[mode]


def _fake_step(sparse):
    """What FlatOptimizer reads of a FusedTrainStep: two entity tables with a dense parameter between and after them."""
    D = 8
    tabs = {'a': torch.nn.Parameter(torch.randn(5, D)), 'b': torch.nn.Parameter(torch.randn(3, D))}
    w0, w1 = torch.nn.Parameter(torch.randn(7)), torch.nn.Parameter(torch.randn(4, 3))
    params = [tabs['a'], w0, tabs['b'], w1]
    step = types.SimpleNamespace()
    step.params, step.device, step.sparse_tables = params, torch.device('cpu'), sparse
    step.flat_grad = torch.zeros(sum(p.numel() for p in params))
    step.err = torch.zeros(1, dtype=torch.int32)
    step.param_epoch = 0
    step.modes = ['a', 'b']
    step.model = types.SimpleNamespace(enc=_Encoder(tabs), emb_dim=D)
    step._refresh_pointers = lambda: None
    return step


@pytest.fixture
def rec(monkeypatch):
    r = _Recorder()
    monkeypatch.setattr(ops, 'lib', lambda: r)
    monkeypatch.setattr(optim._capi, 'check', lambda lib, st, what: None if st == 0 else pytest.fail(what))
    monkeypatch.setattr(torch.cuda, 'device', lambda dev: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda *a: types.SimpleNamespace(cuda_stream=77))
    return r


@pytest.mark.parametrize('kind', ['adam', 'sgd'])
def test_dense_update_entry_points(rec, kind):
    for guard in (True, False):
        del rec.calls[:]
        step = _fake_step(False)
        opt = optim.FlatOptimizer(step, lr=0.01, opt=kind, weight_decay=0.5, guard=guard)
        opt.step()
        (name, args), = rec.calls
        n = step.flat_grad.numel()
        old = ((opt.flat_param.data_ptr(), step.flat_grad.data_ptr(), opt.exp_avg.data_ptr(), opt.exp_avg_sq.data_ptr(), n,
                0.01, 0.9, 0.999, 1e-8, 0.5, 1) if kind == 'adam'
               else (opt.flat_param.data_ptr(), step.flat_grad.data_ptr(), n, 0.01, 0.5))
        if guard:
            assert name == 'mpqe_%s_step_guarded' % kind
            assert args == old + (step.err.data_ptr(), opt.applied.data_ptr(), 77)
            assert opt.applied.dtype == torch.int64 and opt.applied.numel() == 1
        else:
            assert name == 'mpqe_%s_step' % kind
            assert args == old + (77,) and opt.applied is None


def test_sparse_update_entry_points_and_the_counter_goes_last(rec):
    packed = types.SimpleNamespace(touch_ptr=4096, touch_entries=40)
    for guard in (True, False):
        del rec.calls[:]
        step = _fake_step(True)
        opt = optim.FlatOptimizer(step, lr=0.01, sparse_tables=True, guard=guard)
        assert opt.dense_runs == [(40, 7), (71, 12)]              # the parameters between and after the tables
        opt.step(packed)
        sfx = '_guarded' if guard else ''
        assert [c[0] for c in rec.calls] == ['mpqe_adam_step' + sfx, 'mpqe_adam_step' + sfx, 'mpqe_adam_rows_step' + sfx]
        for (name, args), (o, n) in zip(rec.calls[:2], opt.dense_runs):
            assert args[0] == opt.flat_param.data_ptr() + 4 * o and args[4] == n and args[10] == 1
        rows = rec.calls[2][1]
        assert rows[0] == 4096 and rows[1] == 40 and rows[6] == 2 and rows[7] == 8 and rows[12] == 1
        if guard:
            word, counter = step.err.data_ptr(), opt.applied.data_ptr()
            assert [c[1][-3:] for c in rec.calls] == [(word, None, 77), (word, None, 77), (word, counter, 77)]
        else:
            assert [len(c[1]) for c in rec.calls] == [12, 12, 14] and all(c[1][-1] == 77 for c in rec.calls)
        # the plan of the data-parallel row exchange takes the place of the packed step's
        del rec.calls[:]
        opt.step(packed, rows_plan=(8192, 99))
        assert rec.calls[2][1][:2] == (8192, 99) and rec.calls[2][1][12] == 2
    with pytest.raises(ValueError):
        opt.step()


def test_host_step_count_follows_the_device_after_a_clear(rec):
    step = _fake_step(False)
    opt = optim.FlatOptimizer(step, lr=0.01)
    applied = opt.applied
    for want_t in (1, 2):
        opt.step()
        applied += 1                                 # (what the launch does on the device)
        assert rec.calls[-1][1][10] == want_t
    # two updates the device refuses: the host counts on, the device does not
    step.err.fill_(1)
    opt.step()
    opt.step()
    assert opt.t == 4 and rec.calls[-1][1][10] == 4
    clears = ops.flag_clears
    with pytest.raises(IndexError):
        ops.raise_on_flags(step.err)
    assert ops.flag_clears == clears + 1 and int(step.err.item()) == 0
    opt.step()
    applied += 1
    assert opt.t == 3 and rec.calls[-1][1][10] == 3 and opt.steps_applied() == 3
    # a clean word read by the host is no clear: nothing to re-read
    ops.raise_on_flags(step.err)
    assert ops.flag_clears == clears + 1
    # the state dict carries t as before, and the counter follows a load
    sd = opt.state_dict()
    assert sd['t'] == 3
    other = optim.FlatOptimizer(_fake_step(False), lr=0.01)
    other.load_state_dict(sd)
    assert other.t == 3 and other.steps_applied() == 3


def test_clean_path_never_reads_the_counter(rec, monkeypatch):
    step = _fake_step(False)
    opt = optim.FlatOptimizer(step, lr=0.01)

    def no_read(self):
        raise AssertionError('a device-to-host read on the clean path')
    monkeypatch.setattr(torch.Tensor, 'item', no_read)
    for _ in range(3):
        opt.step()
    assert opt.t == 3 and len(rec.calls) == 3


def test_torch_fallback_accepts_and_ignores_guard():
    params = [torch.nn.Parameter(torch.randn(3, 2))]
    for guard in (True, False):
        for cls, torch_cls in ((optim.Adam, torch.optim.Adam), (optim.SGD, torch.optim.SGD)):
            opt = cls(params, lr=0.01, guard=guard)
            assert not opt.flat and isinstance(opt._impl, torch_cls)
            params[0].grad = torch.ones_like(params[0])
            opt.step()
