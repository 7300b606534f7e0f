"""The two vector path decoders without a GPU: the extended float64 oracle (tests/gqe_vec_oracle.py) pinned to the fixtures
the reference wrote (tests/golden/vecdec_*.npz, tools/gen_gqe_vec_golden.py) at the tolerances tests/test_gqe_host.py uses
for the bilinear ones, the module surface against those fixtures (state_dict keys, creation order, negative draws, the
composed path on the CPU), and the decoder factory with and without its keyword."""
import random

import numpy as np
import pytest

from tests import gqe_common as gc
from tests import gqe_vec_common as vc
from tests.gqe_oracle import BWD, FWD

TYPES = ('1chain', '2chain', '3chain', '2inter', '3inter', '3inter_chain', '3chain_inter')


@pytest.fixture(params=vc.case_paths(), ids=vc.case_ids())
def case(request):
    return gc.load_case(request.param)


def test_fixture_set_is_complete():
    ids = vc.case_ids()
    assert len(ids) == 16
    for dec in ('transe', 'bilineardiag'):
        mine = [i for i in ids if i.startswith('vecdec_%s_' % dec)]
        assert len(mine) == 8 and sum(i.endswith('_minsimple') for i in mine) == 1
        for k, qt in enumerate(TYPES):
            hit = [i for i in mine if i in ('vecdec_%s_%s_mean' % (dec, qt), 'vecdec_%s_%s_min' % (dec, qt))]
            assert len(hit) == 1, (dec, qt)
        kinds = [i.rsplit('_', 1)[1] for i in mine if not i.endswith('simple')]
        assert kinds.count('mean') in (3, 4) and kinds.count('min') in (3, 4)
    assert not [i for i in ids if i.startswith('gqe_')]


def test_oracle_matches_the_reference(case):
    a = case.arrays
    inter = case.cfg['inter']
    o = vc.case_oracle(case)
    s = o.forward(case.formula, a['anchors'], a['targets'], a['eval_negs'], a['neg_lengths'], inter)
    assert (a['neg_lengths'] == 0).any()
    np.testing.assert_allclose(s, a['eval_scores'], **FWD)
    np.testing.assert_allclose(o.forward(case.formula, a['anchors'], a['targets'], inter=inter), a['scores_pos'], **FWD)
    np.testing.assert_allclose(o.forward(case.formula, a['anchors'], a['neg_nodes'], inter=inter), a['scores_neg'], **FWD)
    loss = o.margin_loss(case.formula, a['anchors'], a['targets'], a['neg_nodes'], inter)
    np.testing.assert_allclose(loss, float(a['loss']), **FWD)
    grads = case.grads()
    assert set(grads) == set(o.grads)
    used = 0
    for k, g in grads.items():
        np.testing.assert_allclose(o.grads[k], g, err_msg=k, **BWD)
        used += int(k.startswith('path_dec.') and g.any())
    assert used >= 1                        # (the vectors' gradients are in the comparison, not all zero)


def test_state_dict_keys_and_shapes(case):
    from mpqe_amd import BilinearDiagMetapathDecoder, TransEMetapathDecoder
    model = vc.build_model(case)                # (load_state_dict(strict=True) inside)
    sd = model.state_dict()
    assert list(sd.keys()) == case.meta['state_dict_keys']
    for k, v in case.params().items():
        assert tuple(sd[k].shape) == tuple(v.shape), k
    want = {'transe': TransEMetapathDecoder, 'bilinear-diag': BilinearDiagMetapathDecoder}[case.cfg['decoder']]
    assert type(model.path_dec) is want and model.fused is True
    assert set(model.path_dec.vecs) == {(m, name, to) for m in case.relations for (to, name) in case.relations[m]}
    assert all(tuple(v.shape) == (case.D,) for v in model.path_dec.vecs.values())
    assert not hasattr(model.path_dec, 'mats')


def test_negative_draws_follow_the_reference(case):
    model = vc.build_model(case)
    random.seed(case.meta['loss_seed'])
    negs = model.sample_negatives(case.formula, case.queries, case.hard_negatives)
    assert negs == case.arrays['neg_nodes'].tolist()


@pytest.mark.parametrize('name,decoder,inter', [('vecdec_transe_3inter_mean', 'transe', 'mean'),
                                                ('vecdec_bilineardiag_3inter_min', 'bilinear-diag', 'min')])
def test_parameter_creation_order_gives_rng_parity(name, decoder, inter):
    """Same seed, same order of creation -> the reference's initial parameters (the fixtures hold them)."""
    import torch
    from mpqe_amd.data_utils import make_feature_modules
    from mpqe_amd.utils import get_intersection_decoder, get_metapath_decoder
    case = gc.load_case([p for p in vc.case_paths() if p.endswith(name + '.npz')][0])
    torch.manual_seed(case.meta['seed'])
    make_feature_modules(case.ids, case.D, case.num_entities)           # the generator creates the tables first
    graph = gc.CaseGraph(case)
    dims = {m: case.D for m in case.modes}
    path_dec = get_metapath_decoder(graph, dims, decoder, vector_decoders=True)
    inter_dec = get_intersection_decoder(graph, dims, inter)
    params = case.params()
    assert len(list(path_dec.named_parameters())) > 0
    for k, p in path_dec.named_parameters():
        assert torch.equal(p.detach(), params['path_dec.' + k]), k
    for k, p in inter_dec.named_parameters():
        assert torch.equal(p.detach(), params['inter_dec.' + k]), k


def test_factory_with_and_without_the_keyword():
    from mpqe_amd import (BilinearDiagMetapathDecoder, BilinearMetapathDecoder, TransEMetapathDecoder,
                          get_metapath_decoder)
    case = gc.load_case(vc.case_paths()[0])
    graph = gc.CaseGraph(case)
    dims = {m: case.D for m in case.modes}
    for name, cls in (('transe', TransEMetapathDecoder), ('bilinear-diag', BilinearDiagMetapathDecoder)):
        assert type(get_metapath_decoder(graph, dims, name, vector_decoders=True)) is cls
        for kw in ({}, {'vector_decoders': False}):
            with pytest.raises(NotImplementedError) as e:
                get_metapath_decoder(graph, dims, name, **kw)
            assert cls.__name__ in str(e.value) and 'vector_decoders' in str(e.value)
    assert type(get_metapath_decoder(graph, dims, 'bilinear', vector_decoders=True)) is BilinearMetapathDecoder
    with pytest.raises(Exception):
        get_metapath_decoder(graph, dims, 'nonsense', vector_decoders=True)


def test_cpu_parameters_never_take_the_fused_path(case):
    model = vc.build_model(case)
    assert not model._fused_ok(model._plan(case.formula))


_CHAINS = [(p, i) for p, i in zip(vc.case_paths(), vc.case_ids()) if 'inter' not in i]


@pytest.mark.parametrize('path', [p for p, _ in _CHAINS], ids=[i for _, i in _CHAINS])
def test_composed_chain_on_the_cpu_matches_the_fixture(path):
    """The decoders' own forward (plain tensor ops: the composed path) scores a chain on the CPU as the reference did, and
    the gradients are the reference's. (The model's encoder and the intersection decoders run on the library's kernels:
    tests/test_gqe_vec_gpu.py.)"""
    import torch
    case = gc.load_case(path)
    assert len(_CHAINS) == 6
    model = vc.build_model(case)
    a = case.arrays
    f = case.formula
    node_map = torch.from_numpy(a['node_map'])

    def embed(ids, mode):           # DirectEncoder on the CPU (encoders.py:42-43): columns, L2-normalised
        e = model.enc.table(mode)[node_map[torch.as_tensor(ids, dtype=torch.long)]].t()
        return e / e.norm(p=2, dim=0, keepdim=True)

    def scores(nodes):
        return model.path_dec(embed(nodes, f.target_mode), embed(a['anchors'][:, 0], f.anchor_modes[0]), f.rels)
    pos, neg = scores(a['targets']), scores(a['neg_nodes'])
    np.testing.assert_allclose(pos.detach().numpy(), a['scores_pos'], **FWD)
    np.testing.assert_allclose(neg.detach().numpy(), a['scores_neg'], **FWD)
    loss = torch.clamp(1 - (pos - neg), min=0).mean()
    np.testing.assert_allclose(loss.item(), float(a['loss']), **FWD)
    loss.backward()
    grads = case.grads()
    for k, p in model.named_parameters():
        g = np.zeros_like(grads[k]) if p.grad is None else p.grad.numpy()
        np.testing.assert_allclose(g, grads[k], err_msg=k, **BWD)
    # project(): one site, columns in and out
    rel = tuple(f.rels[0])
    x = embed(a['targets'], f.target_mode).detach()
    v = model.path_dec.vecs[rel].detach()
    want = x + v[:, None] if case.cfg['decoder'] == 'transe' else x * v[:, None]
    assert torch.equal(model.path_dec.project(x, rel), want)


def test_programme_carries_operator_and_score():
    from mpqe_amd import ops
    p = ops.gqe_programme(0, [(0, [(0, False)])], 0)
    assert p[7] == 0 and p[27] == 0
    p = ops.gqe_programme(0, [(0, [(0, False), (1, False)])], 0, op='scale', score='dot')
    assert p[7] == 2 and p[27] == 1 and p[10] >> 1 == 0 and p[11] >> 1 == 1
    assert ops.gqe_programme(1, [(0, [(0, True)]), (0, [(1, True)])], 0, 'min', 2, 3, op='translate')[7] == 1
    with pytest.raises(ValueError):
        ops.gqe_programme(0, [(0, [(0, False)])], 0, op='rotate')
    with pytest.raises(ValueError):
        ops.gqe_programme(0, [(0, [(0, False)])], 0, score='l2')
