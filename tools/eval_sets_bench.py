"""Time of the reference's two evaluation metrics (ROC-AUC with one sampled negative per query, percentile rank among all of
a query's negatives; evaluation.eval_auc_queries / eval_perc_queries) over test sets sampled on the device index, two ways:

  list   the sets through QuerySet.queries() -- every id list to the host, one graph.Query per query -- then the list path:
         per batch Python id lists into forward(), the scores back through .cpu().tolist(), the metrics in Python
  sets   the QuerySets themselves: score_ids on device ids, the negatives drawn by the library's sampler, the metrics by
         mpqe_eval_auc / mpqe_eval_counts (csrc/eval.hip); one 8-byte read per AUC, one for the mean percentile
  mixed  kg.MixedQuerySet.from_sets(sets), built once outside the rounds (its time is reported as from_sets_ms): windows
         over a query type's concatenation, queries of different formulas in one scoring call (score_ids_mixed: one launch
         for gqe, two for rgcn), one sampler a type, the per-formula AUCs from one mpqe_eval_auc_segments

on the `small` (480 entities) and `aifb` (2 601 entities) synthetic shapes, for both models (rgcn: RGCNEncoderDecoder, mp
readout; gqe: QueryEncoderDecoder, bilinear paths + mean intersection). The sides run in the same process in alternating
rounds after --warmup rounds of each; a round's time is the host clock around the calls, ending in a device synchronise.
Medians of --rounds rounds, min and max beside them. The two sides score the same queries and negatives; the sampled
negative of the AUC comes from Python's stream on the list side and from the library's on the other, so the AUCs differ
by the draw and the percentiles agree to rounding (both are printed).

  kernels   mpqe_eval_auc on the run's 2 x Q scores and mpqe_eval_counts on its Q lists (device events around blocks of
            calls, through ops.eval_auc / ops.eval_counts: allocation and, for the AUC, the 8-byte read included)

    python tools/eval_sets_bench.py [--kgs small aifb] [--models rgcn gqe] [--per-type 256] [--out profiles/eval_sets_bench.json]
    python tools/eval_sets_bench.py --kgs small --per-type 8192 --min-per-formula 64     # only formulas that fill half a batch
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
SHAPES = {'small': (480, 4, 8)}


def build(kg, which, args, device):
    from mpqe_amd import synthetic
    from mpqe_amd.data_utils import make_feature_modules
    from mpqe_amd.encoders import DirectEncoder
    from mpqe_amd.kg import KGIndex
    from mpqe_amd.model import QueryEncoderDecoder, RGCNEncoderDecoder
    from mpqe_amd.utils import get_intersection_decoder, get_metapath_decoder
    schema = synthetic.make_schema(*(SHAPES.get(kg) or synthetic.KG_SHAPES[kg]), seed=args.seed)
    adj = synthetic.make_adjacency(schema, degree=args.degree, seed=args.seed)
    torch.manual_seed(args.seed)
    graph = synthetic.SchemaGraph(schema, args.embed_dim)
    graph.adj_lists = adj
    fm, node_maps = make_feature_modules(schema.ids, args.embed_dim, schema.num_entities)
    enc = DirectEncoder(None, fm, node_maps)
    if which == 'rgcn':
        model = RGCNEncoderDecoder(graph, enc, readout='mp', num_layers=3, shared_layers=False, adaptive=True, weight_decay=0)
    else:
        dims = {m: args.embed_dim for m in schema.modes}
        model = QueryEncoderDecoder(graph, enc, get_metapath_decoder(graph, dims, 'bilinear'),
                                    get_intersection_decoder(graph, dims, 'mean'))
    model = model.to(device).eval()
    index = KGIndex.from_graph(graph, node_maps, device)
    sets = index.sample_query_sets(QUERY_TYPES, args.per_type, args.seed + 2, neg_sample_max=args.neg_max)
    index.check()
    if args.min_per_formula > 1:            # (the walk meets many formulas with a query or two each: keep the populated ones)
        sets = {f: qs for f, qs in sets.items() if len(qs) >= args.min_per_formula}
        if not sets:
            raise SystemExit('eval_sets_bench: no formula with %d queries at this --per-type' % args.min_per_formula)
    return model, index, sets


def stats(ms):
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def run(kg, which, args, device, emit):
    import kg_answers_bench as kab
    from mpqe_amd import evaluation, ops
    model, index, sets = build(kg, which, args, device)
    Q = sum(len(qs) for qs in sets.values())
    negatives = int(sum(int(qs.neg[0].shape[0]) for qs in sets.values()))
    base = dict(kg=kg, model=which, min_per_formula=args.min_per_formula, queries=Q, formulas=len(sets), negatives=negatives,
                batch_size=args.batch_size, embed_dim=args.embed_dim)
    last = {}
    from mpqe_amd.kg import MixedQuerySet
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mixed = MixedQuerySet.from_sets(sets)
    torch.cuda.synchronize()
    base['from_sets_ms'] = 1e3 * (time.perf_counter() - t0)

    def list_side():
        t0 = time.perf_counter()
        lists = {f: qs.queries() for f, qs in sets.items()}
        t1 = time.perf_counter()
        auc, _ = evaluation.eval_auc_queries(lists, model, batch_size=args.batch_size, seed=0)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        perc = evaluation.eval_perc_queries(lists, model, batch_size=args.batch_size)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        last['list'] = (float(auc), float(perc))
        return [1e3 * (t3 - t0), 1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2)]

    def sets_side():
        t0 = time.perf_counter()
        auc, _ = evaluation.eval_auc_queries(sets, model, batch_size=args.batch_size, seed=0)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        perc = evaluation.eval_perc_queries(sets, model, batch_size=args.batch_size)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        last['sets'] = (float(auc), float(perc))
        return [1e3 * (t2 - t0), 0.0, 1e3 * (t1 - t0), 1e3 * (t2 - t1)]

    def mixed_side():
        t0 = time.perf_counter()
        auc, _ = evaluation.eval_auc_queries(mixed, model, batch_size=args.batch_size, seed=0)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        perc = evaluation.eval_perc_queries(mixed, model, batch_size=args.batch_size)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        last['mixed'] = (float(auc), float(perc))
        return [1e3 * (t2 - t0), 0.0, 1e3 * (t1 - t0), 1e3 * (t2 - t1)]

    sides = {'list': list_side, 'sets': sets_side, 'mixed': mixed_side}
    if args.profile:
        import cProfile
        import pstats
        with torch.no_grad():
            for _ in range(args.warmup):
                sides[args.profile]()
            prof = cProfile.Profile()
            prof.enable()
            sides[args.profile]()
            prof.disable()
        print('cProfile of one %s round, %s / %s' % (args.profile, kg, which))
        pstats.Stats(prof).sort_stats('cumulative').print_stats(25)
        return
    with torch.no_grad():
        for _ in range(args.warmup):
            for side in sides.values():
                side()
        times = {side: [] for side in sides}
        for _ in range(args.rounds):                    # alternating: the sides see the same machine
            for name, side in sides.items():
                times[name].append(side())
    for side in sides:
        t = np.asarray(times[side])
        emit(dict(base, row=side, ms=stats(t[:, 0]), queries_ms=stats(t[:, 1]), auc_ms=stats(t[:, 2]), perc_ms=stats(t[:, 3]),
                  auc=last[side][0], percentile=last[side][1]))
    # the two kernels on scores of the run's size
    g = torch.Generator(device='cpu').manual_seed(args.seed)
    pos = torch.randn(Q, generator=g).to(device)
    neg = torch.randn(Q, generator=g).to(device)
    lengths = torch.cat([qs.neg[1][1:] - qs.neg[1][:-1] for qs in sets.values()])
    offsets = torch.zeros(Q + 1, dtype=torch.int64, device=device)
    torch.cumsum(lengths, 0, out=offsets[1:])
    scores = torch.randn(Q + negatives, generator=g).to(device)
    err = ops.new_error_word(device)
    emit(dict(base, row='kernels', auc_ms=kab.event_timed(lambda: ops.eval_auc(pos, neg), args.warmup, args.rounds),
              counts_ms=kab.event_timed(lambda: ops.eval_counts(scores, offsets, Q, err=err), args.warmup, args.rounds)))
    ops.raise_on_flags(err)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--kgs', nargs='+', default=['small', 'aifb'])
    ap.add_argument('--models', nargs='+', default=['rgcn', 'gqe'])
    ap.add_argument('--per-type', type=int, default=256, help='test queries per query type')
    ap.add_argument('--min-per-formula', type=int, default=1,
                    help='keep only the formulas with at least this many sampled queries (the cost of both sides is per '
                         'formula as well as per query; the default keeps whatever the walk meets)')
    ap.add_argument('--neg-max', type=int, default=100, help='negatives kept per query (the reference\'s neg_sample_max)')
    ap.add_argument('--batch-size', type=int, default=128)
    ap.add_argument('--embed-dim', type=int, default=64)
    ap.add_argument('--degree', type=int, default=2)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=None)
    ap.add_argument('--profile', choices=['list', 'sets', 'mixed'], default=None,
                    help='cProfile of one round of that side per (kg, model) instead of the timing')
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('eval_sets_bench: needs the GPU (a CPU timing says nothing about it)')
    device = torch.device('cuda:0')
    rows = []

    def emit(r):
        rows.append(r)
        print(json.dumps(r), flush=True)
    for kg in args.kgs:
        for which in args.models:
            run(kg, which, args, device, emit)
    if args.profile:
        return rows
    print('| kg | model | queries | formulas | list ms (queries() + AUC + percentile) | sets ms (AUC + percentile) | '
          'mixed ms (AUC + percentile) [min .. max] | list / mixed | sets / mixed | eval_auc ms | eval_counts ms |')
    print('|---|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|')
    keyed = {}
    for r in rows:
        keyed.setdefault((r['kg'], r['model']), {})[r['row']] = r
    for (kg, which), d in keyed.items():
        li, se, mi, ke = d['list'], d['sets'], d['mixed'], d['kernels']
        print('| %s | %s | %d | %d | %.1f (%.1f + %.1f + %.1f) [%.1f .. %.1f] | %.1f (%.1f + %.1f) [%.1f .. %.1f] | '
              '%.1f (%.1f + %.1f) [%.1f .. %.1f] | %.1fx | %.1fx | %.3f | %.3f |'
              % (kg, which, li['queries'], li['formulas'], li['ms'][0], li['queries_ms'][0], li['auc_ms'][0], li['perc_ms'][0],
                 li['ms'][1], li['ms'][2], se['ms'][0], se['auc_ms'][0], se['perc_ms'][0], se['ms'][1], se['ms'][2],
                 mi['ms'][0], mi['auc_ms'][0], mi['perc_ms'][0], mi['ms'][1], mi['ms'][2], li['ms'][0] / mi['ms'][0],
                 se['ms'][0] / mi['ms'][0], ke['auc_ms'][0], ke['counts_ms'][0]))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(dict(args=vars(args), rows=rows), f, indent=1)
    return rows


if __name__ == '__main__':
    main()
