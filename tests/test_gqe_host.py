"""The GQE baseline without a GPU: the float64 oracle (tests/gqe_oracle.py) pinned to the fixtures the reference wrote
(tests/golden/gqe_*.npz, tools/gen_gqe_golden.py), the module surface of QueryEncoderDecoder against those fixtures, and
the argument checks of the new entry points, which answer before any launch."""
import ctypes
import random

import numpy as np
import pytest

from tests import gqe_common as gc
from tests.gqe_oracle import BWD, FWD

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3


@pytest.fixture(params=gc.case_paths(), ids=gc.case_ids())
def case(request):
    return gc.load_case(request.param)


def test_fixture_set_is_complete():
    want = {'gqe_%s_%s' % (qt, inter) for qt in ('1chain', '2chain', '3chain', '2inter', '3inter', '3inter_chain',
                                                  '3chain_inter') for inter in ('mean', 'min')} | {'gqe_2inter_minsimple'}
    assert set(gc.case_ids()) == want


def test_oracle_matches_the_reference(case):
    a = case.arrays
    inter = case.cfg['inter']
    o = gc.case_oracle(case)
    s = o.forward(case.formula, a['anchors'], a['targets'], a['eval_negs'], a['neg_lengths'], inter)
    assert (a['neg_lengths'] == 0).any()
    np.testing.assert_allclose(s, a['eval_scores'], **FWD)
    np.testing.assert_allclose(o.forward(case.formula, a['anchors'], a['targets'], inter=inter), a['scores_pos'], **FWD)
    np.testing.assert_allclose(o.forward(case.formula, a['anchors'], a['neg_nodes'], inter=inter), a['scores_neg'], **FWD)
    loss = o.margin_loss(case.formula, a['anchors'], a['targets'], a['neg_nodes'], inter)
    np.testing.assert_allclose(loss, float(a['loss']), **FWD)
    grads = case.grads()
    assert set(grads) == set(o.grads)
    for k, g in grads.items():
        np.testing.assert_allclose(o.grads[k], g, err_msg=k, **BWD)


def test_state_dict_keys_and_shapes(case):
    model = gc.build_model(case)                # (load_state_dict(strict=True) inside)
    sd = model.state_dict()
    assert list(sd.keys()) == case.meta['state_dict_keys']
    for k, v in case.params().items():
        assert tuple(sd[k].shape) == tuple(v.shape), k
    assert model.fused is True
    inter = case.cfg['inter']
    if inter.endswith('simple'):
        assert not list(model.inter_dec.parameters())
    else:
        assert set(model.inter_dec.pre_mats) == set(case.modes) == set(model.inter_dec.post_mats)
    assert set(model.path_dec.mats) == {(m, name, to) for m in case.relations for (to, name) in case.relations[m]}


def test_negative_draws_follow_the_reference(case):
    model = gc.build_model(case)
    random.seed(case.meta['loss_seed'])
    negs = model.sample_negatives(case.formula, case.queries, case.hard_negatives)
    assert negs == case.arrays['neg_nodes'].tolist()


def test_hard_negatives_on_a_chain_raise_the_reference_text():
    case = gc.load_case([p for p in gc.case_paths() if p.endswith('gqe_2chain_mean.npz')][0])
    model = gc.build_model(case)
    with pytest.raises(Exception) as e:
        model.margin_loss(case.formula, case.queries, hard_negatives=True)
    assert str(e.value) == 'Hard negative examples can only be used with intersection queries'


def test_decoders_not_built_raise():
    from mpqe_amd import get_intersection_decoder, get_metapath_decoder
    case = gc.load_case(gc.case_paths()[0])
    graph = gc.CaseGraph(case)
    dims = {m: case.D for m in case.modes}
    for name, cls in (('transe', 'TransEMetapathDecoder'), ('bilinear-diag', 'BilinearDiagMetapathDecoder')):
        with pytest.raises(NotImplementedError) as e:
            get_metapath_decoder(graph, dims, name)
        assert cls in str(e.value)
    with pytest.raises(Exception):
        get_metapath_decoder(graph, dims, 'nonsense')
    with pytest.raises(Exception):
        get_intersection_decoder(graph, dims, 'nonsense')
    import torch
    from mpqe_amd import SetIntersection, SimpleSetIntersection
    for name, cls, agg in (('mean', SetIntersection, torch.mean), ('min', SetIntersection, torch.min),
                           ('mean-simple', SimpleSetIntersection, torch.mean), ('min-simple', SimpleSetIntersection, torch.min)):
        dec = get_intersection_decoder(graph, dims, name)
        assert type(dec) is cls and dec.agg_func is agg


def test_parameter_creation_order_gives_rng_parity():
    """Same seed, same order of creation -> the reference's initial parameters (the fixtures hold them)."""
    import torch
    from mpqe_amd.data_utils import make_feature_modules
    from mpqe_amd.utils import get_intersection_decoder, get_metapath_decoder
    case = gc.load_case([p for p in gc.case_paths() if p.endswith('gqe_3inter_min.npz')][0])
    torch.manual_seed(case.meta['seed'])
    make_feature_modules(case.ids, case.D, case.num_entities)           # the generator creates the tables first
    graph = gc.CaseGraph(case)
    dims = {m: case.D for m in case.modes}
    path_dec = get_metapath_decoder(graph, dims, 'bilinear')
    inter_dec = get_intersection_decoder(graph, dims, 'min')
    params = case.params()
    for k, p in path_dec.named_parameters():
        assert torch.equal(p.detach(), params['path_dec.' + k]), k
    for k, p in inter_dec.named_parameters():
        assert torch.equal(p.detach(), params['inter_dec.' + k]), k


# ---------------------------------------------------------------------------------------------- argument checks, no launch
def _libs():
    from mpqe_amd import _lib
    from tests.kernel_backend import EmuBackend
    return [('emu', EmuBackend().lib), ('product', _lib.load())]


@pytest.mark.parametrize('which', ['emu', 'product'])
def test_entry_points_refuse_before_any_launch(which):
    """Device pointers are made-up addresses: a call that launched anything with them would fault. Every call here must
    answer from its checks."""
    from mpqe_amd import ops
    lib = dict(_libs())[which]
    D, B, n = 32, 5, 9
    prog = np.ascontiguousarray(ops.gqe_programme(1, [(0, [(0, True)]), (0, [(1, True)])], 0, 'min', 2, 3))
    fake = 0x10000
    tabs = (ctypes.c_void_p * 1)(fake)
    rows = (ctypes.c_int64 * 1)(10)
    mats = (ctypes.c_void_p * 4)(fake, fake, fake, fake)
    need = lib.mpqe_gqe_workspace_bytes(prog.ctypes.data, B, n, D)
    assert need > 0

    def fwd(prog=prog, tabs=tabs, num_mats=4, D=D, p_ids=fake, p_rows=B, e_rows=n, neg_off=fake, n=n, scores=fake, ws=fake,
            wb=need, save=1):
        return lib.mpqe_gqe_fwd(prog.ctypes.data if prog is not None else None, tabs, rows, 1, fake, 11, mats, num_mats, D,
                                p_ids, p_rows, fake, e_rows, None, neg_off, n, 1e-8, save, scores, ws, wb, None, None)

    def bwd(gs=fake, wb=need, gt=(ctypes.c_void_p * 1)(fake), gm=(ctypes.c_void_p * 4)(fake, fake, fake, fake), D=D):
        return lib.mpqe_gqe_bwd(prog.ctypes.data, tabs, rows, 1, fake, 11, mats, 4, D, fake, B, fake, n, None, fake, n, 1e-8,
                                gs, gt, gm, fake, wb, None, None)

    assert fwd(prog=None) == INVALID
    assert fwd(tabs=None) == INVALID
    assert fwd(p_ids=None) == INVALID
    assert fwd(scores=None) == INVALID
    assert fwd(p_rows=0) == INVALID
    assert fwd(e_rows=n - 1) == INVALID                 # intersection form: one row of the other side per score
    assert fwd(neg_off=None) == INVALID                 # negatives without their offsets
    assert fwd(num_mats=3) == INVALID                   # the programme names matrix 3
    assert fwd(ws=None) == INVALID and fwd(ws=fake + 4) == INVALID
    assert fwd(D=24) == UNSUPPORTED and fwd(D=272) == UNSUPPORTED
    assert fwd(wb=need - 1) == WORKSPACE
    bad = prog.copy()
    bad[1] = 4                                          # four branches
    assert fwd(prog=bad) == INVALID
    bad = prog.copy()
    bad[0] = 0                                          # chain form with an intersection programme's sizes
    assert fwd(prog=bad) == INVALID
    assert bwd(gs=None) == INVALID and bwd(gt=None) == INVALID and bwd(gm=None) == INVALID
    assert bwd(D=24) == UNSUPPORTED
    assert bwd(wb=need - 1) == WORKSPACE
    assert lib.mpqe_gqe_workspace_bytes(prog.ctypes.data, B, n, 24) == 0
    assert lib.mpqe_gqe_workspace_bytes(None, B, n, D) == 0
    assert lib.mpqe_branch_agg_fwd(None, fake, None, 8, 0, fake, None) == INVALID
    assert lib.mpqe_branch_agg_fwd(fake, fake, None, 8, 2, fake, None) == INVALID
    assert lib.mpqe_branch_agg_bwd(fake, fake, None, 8, 1, None, fake, fake, None, None) == INVALID


def test_unsupported_shapes_take_the_composed_path():
    """D = 24 is outside the fused kernel (a multiple of 16 up to 256): the model must not hand it to ops.gqe_scores."""
    from mpqe_amd import ops
    assert ops.gqe_supported(16) and ops.gqe_supported(256) and ops.gqe_supported(48)
    assert not ops.gqe_supported(24) and not ops.gqe_supported(272) and not ops.gqe_supported(8)
    case = gc.load_case(gc.case_paths()[0])
    model = gc.build_model(case)
    assert not model._fused_ok(model._plan(case.formula))          # (parameters on the CPU: never the fused path)
