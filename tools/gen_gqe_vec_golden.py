"""TEST INFRASTRUCTURE ONLY, run where a checkout of the reference exists -- generates
tests/golden/vecdec_<decoder>_<type>_<inter>.npz, the sibling of tools/gen_gqe_golden.py for the reference's two vector path
decoders (TransEMetapathDecoder, BilinearDiagMetapathDecoder): it IMPORTS the reference and runs it on the tiny synthetic
KG, with the stand-ins and the `min` wrapper of that tool. Only inputs and expected outputs are written.

    MPQE_REFERENCE=<checkout of the reference> python tools/gen_gqe_vec_golden.py

Each fixture holds what a gqe_*.npz fixture holds, plus cfg.decoder ('transe' | 'bilinear-diag'). Per decoder: the seven
query types alternating mean / min, and one min-simple case. D = 16, B = 5. (The names do not start with gqe_: the
bilinear fixture tests glob that prefix.)
"""
import json
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_gqe_golden as base  # noqa: E402

DECODERS = ('transe', 'bilinear-diag')


def case_name(decoder, query_type, inter):
    return 'vecdec_%s_%s_%s' % (decoder.replace('-', ''), query_type.replace('-', ''), inter.replace('-', ''))


def run_case(decoder, query_type, inter, seed, D=16, B=5):
    rmodel, rdec, rgraph, renc = base._reference()
    from mpqe_amd import synthetic
    name = case_name(decoder, query_type, inter)
    schema = synthetic.make_schema(*synthetic.KG_SHAPES['tiny'], seed=seed)
    adj = synthetic.make_adjacency(schema, degree=2, seed=seed)
    torch.manual_seed(seed)
    node_map = torch.full((schema.num_entities + 1,), -1, dtype=torch.long)
    for m in schema.modes:
        for i, n in enumerate(schema.ids[m].tolist()):
            node_map[n] = i
    feature_modules = {m: torch.nn.Embedding(len(schema.ids[m]) + 1, D) for m in schema.modes}
    for m in schema.modes:
        feature_modules[m].weight.data.normal_(0, 1. / D)
    features = lambda nodes, mode: feature_modules[mode](node_map[nodes])       # noqa: E731
    dims = {m: D for m in schema.modes}
    graph = rgraph.Graph(features, dims, schema.relations, adj)
    enc = renc.DirectEncoder(graph.features, feature_modules)
    path_dec = {'transe': rdec.TransEMetapathDecoder, 'bilinear-diag': rdec.BilinearDiagMetapathDecoder}[decoder](
        graph.relations, dims)
    # (the `min` wrapper of tools/gen_gqe_golden.py: today's torch.min(dim=...) returns a named tuple)
    agg = torch.mean if inter.startswith('mean') else (lambda x, dim: torch.min(x, dim=dim)[0])
    inter_dec = rdec.SimpleSetIntersection(agg_func=agg) if inter.endswith('simple') else \
        rdec.SetIntersection(dims, dims, agg_func=agg)
    model = rmodel.QueryEncoderDecoder(graph, enc, path_dec, inter_dec)

    rng = np.random.RandomState(2000 + seed)
    my_formula = synthetic.sample_formula(schema, query_type, rng)
    my_queries = synthetic.sample_queries(schema, my_formula, B, rng, n_neg=3, n_hard=2)
    queries = [rgraph.Query(q.query_graph, q.neg_samples, q.hard_neg_samples, 100, True) for q in my_queries]
    formula = queries[0].formula
    targets = [q.target_node for q in queries]

    eval_negs = [n for q, l in zip(queries, base.NEG_LENGTHS) for n in q.neg_samples[:l]]
    with torch.no_grad():
        eval_scores = model.forward(formula, queries, targets, neg_nodes=eval_negs, neg_lengths=base.NEG_LENGTHS)

    hard = 'inter' in query_type and seed % 2 == 1
    loss_seed = 777 + seed
    random.seed(loss_seed)
    if hard:
        neg_nodes = [random.choice(q.hard_neg_samples) for q in queries]
    elif query_type == '1-chain':
        neg_nodes = [random.choice(graph.full_lists[formula.target_mode]) for _ in queries]
    else:
        neg_nodes = [random.choice(q.neg_samples) for q in queries]
    random.seed(loss_seed)
    model.zero_grad()
    loss = model.margin_loss(formula, queries, hard_negatives=hard)
    loss.backward()
    with torch.no_grad():
        scores_pos = model.forward(formula, queries, targets)
        scores_neg = model.forward(formula, queries, neg_nodes)

    arrays = {}
    for k, v in model.state_dict().items():
        arrays['param/' + k] = v.detach().numpy()
    for k, p in model.named_parameters():
        arrays['grad/' + k] = (p.grad if p.grad is not None else torch.zeros_like(p)).detach().numpy()
    arrays.update({
        'node_map': node_map.numpy(), 'targets': np.array(targets, dtype=np.int64),
        'anchors': np.array([q.anchor_nodes for q in queries], dtype=np.int64),
        'eval_negs': np.array(eval_negs, dtype=np.int64), 'neg_lengths': np.array(base.NEG_LENGTHS, dtype=np.int64),
        'eval_scores': eval_scores.numpy(), 'neg_nodes': np.array(neg_nodes, dtype=np.int64),
        'scores_pos': scores_pos.numpy(), 'scores_neg': scores_neg.numpy(),
        'loss': np.array(loss.item(), dtype=np.float64)})
    meta = {'name': name, 'query_type': query_type, 'cfg': {'inter': inter, 'decoder': decoder}, 'D': D, 'B': B, 'seed': seed,
            'loss_seed': loss_seed, 'hard_negatives': hard,
            'schema': {'modes': schema.modes, 'relations': {m: base._jsonable(v) for m, v in schema.relations.items()},
                       'ids': {m: schema.ids[m].tolist() for m in schema.modes}, 'num_entities': schema.num_entities},
            'mode_weights_order': list(graph.mode_weights.keys()), 'num_relations': len(graph.rel_edges),
            'mode_ids': {}, 'rel_ids': [], 'formula_rels': base._jsonable(formula.rels),
            'state_dict_keys': list(model.state_dict().keys()),
            'queries': [{'graph': base._jsonable(q.query_graph), 'neg': base._jsonable(q.neg_samples),
                         'hard': base._jsonable(q.hard_neg_samples)} for q in my_queries],
            'full_list_target_mode': base._jsonable(graph.full_lists[formula.target_mode]), 'n_layer_calls': 0}
    arrays['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    os.makedirs(base.OUT, exist_ok=True)
    np.savez_compressed(os.path.join(base.OUT, name + '.npz'), **arrays)
    return name, loss.item()


def cases():
    out = []
    for d, decoder in enumerate(DECODERS):
        for k, qt in enumerate(base.QUERY_TYPES):
            out.append((decoder, qt, 'mean' if (k + d) % 2 == 0 else 'min', 40 + 10 * d + k))
        out.append((decoder, '2-inter' if d == 0 else '3-inter', 'min-simple', 60 + d))
    return out


if __name__ == '__main__':
    for decoder, qt, inter, seed in cases():
        print('%-40s loss=%.6f' % run_case(decoder, qt, inter, seed))
