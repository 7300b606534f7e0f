"""Time of the exact answers of a batch of queries on the knowledge graph -- kg.KGIndex.answers + KGAnswers.exclusion_csr
(csrc/kg.hip) -- beside the host path it replaces: synthetic._answers per query (Python sets) and the numpy CSR build of
_EntityRanking._rank_rows (id translation, unique, searchsorted, upload), timed on this machine's CPU. B = 512 queries per
query type, on

  aifb   the AIFB-shaped graph (2 601 entities, synthetic.make_adjacency): both paths, and one evaluation.eval_rank_queries
         pass over the seven types with known_answers = the index / = the dict of sets (the dict's own build timed apart)
  am     an AM-shaped random graph (372 584 entities, 5 modes, 19 relation names) through KGIndex.from_edges: no Python
         adjacency exists, so there is no host row -- the absolute time and the bytes of bitmap per query. Its queries
         are grounded by random walks over the index's CSRs, so the answer sets are not empty

Rows: `device` the whole call from Query objects to the CSR on the device (host clock, ends in a synchronise); `kernel`
mpqe_kg_answers alone on prepared anchor rows (device events); `host` the replaced path. Medians of --blocks blocks after
--warmup calls; min and max beside them. One JSON line per row, then the table.

    python tools/kg_answers_bench.py [--kgs aifb am] [--batch 512] [--dim 128]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

QUERY_TYPES = ['1-chain', '2-chain', '3-chain', '2-inter', '3-inter', '3-inter_chain', '3-chain_inter']


def host_timed(fn, warmup, blocks):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(blocks):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def event_timed(fn, warmup, blocks, iters=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(blocks):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / iters)
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def random_edges(schema, degree, seed):
    """{relation: (src ids, dst ids)} closed under inverse: `degree` random neighbours per source entity, as arrays"""
    from mpqe_amd.graph import reverse_relation
    rng = np.random.RandomState(seed + 17)
    edges = {}
    for rel in schema.typed_relations():
        if rel in edges:
            continue
        src = np.repeat(schema.ids[rel[0]], degree)
        dst = schema.ids[rel[2]][rng.randint(len(schema.ids[rel[2]]), size=src.shape[0])]
        edges[rel] = (src, dst)
        inv = reverse_relation(rel)
        if inv != rel:
            edges[inv] = (dst, src)
        else:
            edges[rel] = (np.concatenate([src, dst]), np.concatenate([dst, src]))
    return edges


def grounded_queries(index, schema, formula, count, rng):
    """`count` Query objects whose target really answers them, by random walks over the index's own CSRs (host copies):
    what synthetic.sample_grounded_queries does on a Python adjacency, for graphs that have none."""
    from mpqe_amd import synthetic
    from mpqe_amd.graph import Query
    host = {}

    def step(rel, rows):
        i = index.rel_index[tuple(rel)]
        if i not in host:
            host[i] = (index.offsets[i].cpu().numpy(), index.rows[i].cpu().numpy())
        off, nb = host[i]
        at = np.maximum(rows, 0)
        deg = np.where(rows >= 0, off[at + 1] - off[at], 0)
        pick = off[at] + rng.randint(0, 2 ** 31 - 1, size=rows.shape[0]) % np.maximum(deg, 1)
        return np.where(deg > 0, nb[np.minimum(pick, nb.shape[0] - 1)], -1)
    qt, rels = formula.query_type, formula.rels
    n = index.row_ids_host[formula.target_mode].shape[0]
    t = rng.randint(0, n, size=4 * count + 64)
    t = np.where(index.row_ids_host[formula.target_mode][t] >= 0, t, -1)
    if qt.endswith('-chain'):
        walk = [t]
        for r in rels:
            walk.append(step(r, walk[-1]))
        anchors, variables = [walk[-1]], walk[1:-1]
        anchor_rels, var_rels = [rels[-1]], rels[:-1]
    elif qt.endswith('-inter'):
        anchors, variables = [step(r, t) for r in rels], []
        anchor_rels, var_rels = list(rels), []
    elif qt == '3-inter_chain':
        v = step(rels[1][0], t)
        anchors, variables = [step(rels[0], t), step(rels[1][1], v)], [v]
        anchor_rels, var_rels = [rels[0], rels[1][1]], [rels[1][0]]
    else:
        v = step(rels[0], t)
        anchors, variables = [step(rels[1][0], v), step(rels[1][1], v)], [v]
        anchor_rels, var_rels = [rels[1][0], rels[1][1]], [rels[0]]
    good = np.nonzero(np.all(np.stack([t] + anchors + variables) >= 0, axis=0))[0][:count]
    if good.shape[0] < count:
        raise RuntimeError('too few grounded queries of %s' % (formula,))
    ids = lambda rel_or_mode, rows: index.row_ids_host[rel_or_mode][rows[good]]           # noqa: E731
    tid = ids(formula.target_mode, t)
    aid = [ids(r[2], a) for r, a in zip(anchor_rels, anchors)]
    vid = [ids(r[2], v) for r, v in zip(var_rels, variables)]
    return [Query(synthetic.query_graph_tuple(formula, int(tid[i]), [int(a[i]) for a in aid], [int(v[i]) for v in vid]),
                  keep_graph=True) for i in range(count)]


def host_exclusion(index, adj, formula, queries, device):
    """the replaced path: the sets in Python, then _rank_rows' CSR build and upload"""
    from mpqe_amd import synthetic
    exclude = [list(synthetic._answers(adj, formula, list(q.anchor_nodes))[0]) for q in queries]
    B = len(queries)
    mode = formula.target_mode
    n = index.row_ids_host[mode].shape[0]
    holes = np.nonzero(index.row_ids_host[mode] < 0)[0].astype(np.int64)
    lens = np.fromiter((len(e) for e in exclude), dtype=np.int64, count=B)
    flat = np.fromiter((x for e in exclude for x in e), dtype=np.int64, count=int(lens.sum()))
    rows = np.concatenate([index._rows_of(mode, flat), np.tile(holes, B)])
    owner = np.concatenate([np.repeat(np.arange(B, dtype=np.int64), lens), np.repeat(np.arange(B, dtype=np.int64), holes.size)])
    keys = np.unique(owner * (n + 1) + rows)
    off = np.searchsorted(keys, np.arange(B + 1, dtype=np.int64) * (n + 1)).astype(np.int64)
    return torch.from_numpy(off).to(device), torch.from_numpy(keys % (n + 1)).to(device)


def run_kg(kg, args, device, emit):
    from mpqe_amd import evaluation, synthetic
    from mpqe_amd.data_utils import make_feature_modules
    from mpqe_amd.kg import KGIndex
    schema = synthetic.make_schema(*synthetic.KG_SHAPES[kg], seed=args.seed)
    _, node_maps = make_feature_modules(schema.ids, 4, schema.num_entities)
    has_adj = kg == 'aifb'
    t0 = time.perf_counter()
    if has_adj:
        adj = synthetic.make_adjacency(schema, degree=args.degree, seed=args.seed)
        graph = synthetic.SchemaGraph(schema, 4)
        graph.adj_lists = adj
        index = KGIndex.from_graph(graph, node_maps, device)
    else:
        adj = None
        index = KGIndex.from_edges(schema, random_edges(schema, args.am_degree, args.seed), node_maps, device)
    torch.cuda.synchronize()
    emit(dict(kg=kg, row='index_build', seconds=time.perf_counter() - t0, entities=schema.num_entities,
              edges=int(sum(r.numel() for r in index.rows)), widest_mode_rows=int(index.mode_rows.max())))
    rng = np.random.RandomState(args.seed + 3)
    test_queries = {}
    for qt in QUERY_TYPES:
        formula = synthetic.sample_formula(schema, qt, rng)
        if has_adj:
            queries = synthetic.sample_grounded_queries(schema, adj, formula, args.batch, rng, n_neg=1, n_hard=1)
        else:
            queries = grounded_queries(index, schema, formula, args.batch, rng)
        test_queries[formula] = queries
        prog, _ = index.programme(formula)
        rows = index.anchor_rows(formula, queries)
        ans = index.answers(formula, queries, hard=True)
        n = ans.n
        base = dict(kg=kg, query_type=qt, batch=args.batch, target_rows=n, bitmap_bytes_per_query=4 * ((n + 31) // 32),
                    mean_answers=float(ans.counts[0].double().mean().item()), mean_hard=float(ans.counts[1].double().mean().item()))

        def device_path():
            return index.answers(formula, queries).exclusion_csr()
        emit(dict(base, row='device', ms=host_timed(device_path, args.warmup, args.blocks)))
        emit(dict(base, row='kernel', ms=event_timed(lambda: index.answers_of_rows(formula, prog, rows), args.warmup, args.blocks)))
        emit(dict(base, row='kernel_hard', ms=event_timed(lambda: index.answers_of_rows(formula, prog, rows, hard=True),
                                                          args.warmup, args.blocks)))
        if has_adj:
            off_d, rows_d = device_path()
            off_h, rows_h = host_exclusion(index, adj, formula, queries, device)
            assert torch.equal(off_d, off_h) and torch.equal(rows_d, rows_h), 'the two paths disagree'
            emit(dict(base, row='host', ms=host_timed(lambda: host_exclusion(index, adj, formula, queries, device),
                                                      1, max(3, args.blocks // 4))))
    index.check()
    # one filtered evaluation pass over the seven types, both ways (GQE baseline, untrained: the cost does not depend on it)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import answer_bench
    _, model = answer_bench.build_gqe(kg, args.dim, 'mean', seed=args.seed)          # (the same schema: same seed)
    model = model.to(device).eval()
    total = sum(len(v) for v in test_queries.values())

    def by_index():
        return evaluation.eval_rank_queries(test_queries, model, batch_size=args.batch, ks=(10,), known_answers=index)
    got = by_index()
    emit(dict(kg=kg, row='eval_index', queries=total, ms=host_timed(by_index, 1, 5), mrr=got['mrr']))
    if has_adj:
        t0 = time.perf_counter()
        known = {q: synthetic._answers(adj, f, list(q.anchor_nodes))[0] for f, qs in test_queries.items() for q in qs}
        dict_ms = 1e3 * (time.perf_counter() - t0)

        def by_dict():
            return evaluation.eval_rank_queries(test_queries, model, batch_size=args.batch, ks=(10,), known_answers=known)
        assert by_dict() == got, 'the two evaluations disagree'
        emit(dict(kg=kg, row='eval_dict', queries=total, ms=host_timed(by_dict, 1, 5), dict_build_ms=dict_ms))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--kgs', nargs='+', default=['aifb', 'am'])
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--dim', type=int, default=128)
    ap.add_argument('--degree', type=int, default=2, help='neighbours per entity and relation on the graphs with an adjacency')
    ap.add_argument('--am-degree', type=int, default=8, help='... on the AM-shaped random graph')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--blocks', type=int, default=20)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('kg_answers_bench: needs the GPU (a CPU timing says nothing about it)')
    device = torch.device('cuda:0')
    rows = []

    def emit(r):
        rows.append(r)
        print(json.dumps(r), flush=True)
    for kg in args.kgs:
        run_kg(kg, args, device, emit)
    print('| kg | query type | rows | B/query | mean answers | device ms | kernel ms | kernel+hard ms | host ms |')
    print('|---|---|---|---|---|---|---|---|---|')
    keyed = {}
    for r in rows:
        if 'query_type' in r:
            keyed.setdefault((r['kg'], r['query_type']), {})[r['row']] = r
    for (kg, qt), d in keyed.items():
        b = d['device']
        host = '%.2f' % d['host']['ms'][0] if 'host' in d else 'none'
        print('| %s | %s | %d | %d | %.1f | %.3f | %.3f | %.3f | %s |' % (kg, qt, b['target_rows'], b['bitmap_bytes_per_query'],
                                                                          b['mean_answers'], b['ms'][0], d['kernel']['ms'][0],
                                                                          d['kernel_hard']['ms'][0], host))
    return rows


if __name__ == '__main__':
    main()
