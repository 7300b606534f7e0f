"""Time of sampling grounded queries and their negatives on the device index -- kg.KGIndex.sample_queries (the walk,
csrc/kg_sample.hip) and kg.KGIndex.sample_query_sets (walk + exact answers + at most 100 negatives / hard negatives per
query) -- beside the host stand-in it replaces, synthetic.sample_grounded_queries (one walk per query in Python, the whole
target mode scanned per query for the negatives), timed on this machine's CPU in one thread. Per query type, for --counts
queries, on

  aifb   the AIFB-shaped graph (2 601 entities, synthetic.make_adjacency): both sides
  am     an AM-shaped random graph (372 584 entities) through KGIndex.from_edges: no Python adjacency exists, no host row

Rows: `walk` mpqe_kg_sample_queries alone for `count` slots (device events around blocks of calls); `sets` the whole
sample_query_sets call until `count` queries of the type are kept (host clock, ends in a device synchronise; its formulas
are whichever the walk meets, so it is many small answers() calls -- the row says how many); `batched` the same call with
batched=True (one answers_mixed launch per type and round, in the same process, timed the same way; sections_ms: one further
call synchronised between its sections); `host` the stand-in for ONE
formula, at most --host-cap queries (its cost is per query; the row gives microseconds per query for both sides). The two
sides do not sample the same distribution: the host draws a target uniformly in the formula's mode and 8 negatives with
replacement, the device follows the reference's walk and keeps up to 100 distinct negatives. Medians of --blocks timed
calls after --warmup (counts above 10 000: 3 calls of `sets`, warmed by the smaller count); min and max beside them. One JSON line per row, then the table.

    python tools/kg_sample_bench.py [--kgs aifb am] [--counts 1000 100000] [--out profiles/kg_sample_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

QUERY_TYPES = ['1-chain', '2-chain', '3-chain', '2-inter', '3-inter', '3-inter_chain', '3-chain_inter']


def run_kg(kg, args, device, emit):
    import kg_answers_bench as kab
    from mpqe_amd import synthetic
    from mpqe_amd.data_utils import make_feature_modules
    from mpqe_amd.kg import KGIndex
    schema = synthetic.make_schema(*synthetic.KG_SHAPES[kg], seed=args.seed)
    _, node_maps = make_feature_modules(schema.ids, 4, schema.num_entities)
    has_adj = kg == 'aifb'
    if has_adj:
        adj = synthetic.make_adjacency(schema, degree=args.degree, seed=args.seed)
        graph = synthetic.SchemaGraph(schema, 4)
        graph.adj_lists = adj
        index = KGIndex.from_graph(graph, node_maps, device)
    else:
        adj = None
        index = KGIndex.from_edges(schema, kab.random_edges(schema, args.am_degree, args.seed), node_maps, device)
    edges = int(sum(r.numel() for r in index.rows))
    rng = np.random.RandomState(args.seed + 3)
    formulas = {qt: synthetic.sample_formula(schema, qt, rng) for qt in QUERY_TYPES}         # (the host side's)
    for count in args.counts:
        blocks, warm = (args.blocks, 1) if count <= 10000 else (3, 0)      # (the large count runs after the small one)
        for qt in QUERY_TYPES:
            base = dict(kg=kg, query_type=qt, count=count, edges=edges, relations=len(index.rels))
            rec = index.sample_queries(qt, count, 1)
            found = float(rec[:, 0].double().mean().item())
            emit(dict(base, row='walk', found=found,
                      ms=kab.event_timed(lambda: index.sample_queries(qt, count, 1), args.warmup, blocks, iters=5)))
            last = {}

            def sets():
                last['sets'] = index.sample_query_sets([qt], count, args.seed + 1, neg_sample_max=100)
            ms = kab.host_timed(sets, warm, blocks)
            kept = sum(len(s) for s in last['sets'].values())
            emit(dict(base, row='sets', kept=kept, formulas=len(last['sets']), ms=ms, us_per_query=1e3 * ms[0] / max(kept, 1),
                      negatives=int(sum(int(s.neg[0].shape[0]) for s in last['sets'].values()))))

            def batched():
                last['batched'] = index.sample_query_sets([qt], count, args.seed + 1, neg_sample_max=100, batched=True)
            ms = kab.host_timed(batched, warm, blocks)
            kept = sum(len(s) for s in last['batched'].values())
            index.section_times = {}                # one more call, synchronised between its sections: where the time goes
            batched()
            sections, index.section_times = {k: 1e3 * v for k, v in index.section_times.items()}, None
            emit(dict(base, row='batched', kept=kept, formulas=len(last['batched']), ms=ms,
                      us_per_query=1e3 * ms[0] / max(kept, 1), sections_ms=sections,
                      negatives=int(sum(int(s.neg[0].shape[0]) for s in last['batched'].values()))))
            if has_adj:
                formula = formulas[qt]
                n = min(count, args.host_cap)
                t = []
                for _ in range(3 if n <= 1000 else 1):
                    t0 = time.perf_counter()
                    synthetic.sample_grounded_queries(schema, adj, formula, n, np.random.RandomState(5))
                    t.append(1e3 * (time.perf_counter() - t0))
                emit(dict(base, row='host', queries=n, ms=(float(np.median(t)), float(np.min(t)), float(np.max(t))),
                          us_per_query=1e3 * float(np.median(t)) / n))
    index.check()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--kgs', nargs='+', default=['aifb', 'am'])
    ap.add_argument('--counts', nargs='+', type=int, default=[1000, 100000])
    ap.add_argument('--degree', type=int, default=2, help='neighbours per entity and relation on the graph with an adjacency')
    ap.add_argument('--am-degree', type=int, default=8, help='... on the AM-shaped random graph')
    ap.add_argument('--host-cap', type=int, default=10000, help='the host stand-in is timed on at most this many queries')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--blocks', type=int, default=9)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('kg_sample_bench: needs the GPU (a CPU timing says nothing about it)')
    device = torch.device('cuda:0')
    rows = []

    def emit(r):
        rows.append(r)
        print(json.dumps(r), flush=True)
    for kg in args.kgs:
        run_kg(kg, args, device, emit)
    host = dict(cpu_count=os.cpu_count(), threads=1, python=sys.version.split()[0])
    try:
        with open('/proc/cpuinfo') as f:
            host['cpu'] = [l.split(':', 1)[1].strip() for l in f if l.startswith('model name')][0]
    except (OSError, IndexError):
        host['cpu'] = 'unknown'
    print(json.dumps(dict(row='host_cpu', **host)), flush=True)
    print('| kg | query type | count | walk ms | found | sets ms | kept | formulas | sets us/query | batched ms | '
          'batched us/query | host us/query |')
    print('|---|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|')
    keyed = {}
    for r in rows:
        keyed.setdefault((r['kg'], r['count'], r['query_type']), {})[r['row']] = r
    for (kg, count, qt), d in keyed.items():
        h = '%.1f' % d['host']['us_per_query'] if 'host' in d else 'none'
        s = d['sets']
        b = d['batched']
        print('| %s | %s | %d | %.3f (%.3f - %.3f) | %.2f | %.1f (%.1f - %.1f) | %d | %d | %.2f | %.1f (%.1f - %.1f) | %.2f | %s |'
              % ((kg, qt, count) + tuple(d['walk']['ms']) + (d['walk']['found'],) + tuple(s['ms']) +
                 (s['kept'], s['formulas'], s['us_per_query']) + tuple(b['ms']) + (b['us_per_query'], h)))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(dict(host=host, args=vars(args), rows=rows), f, indent=1)
    return rows


if __name__ == '__main__':
    main()
