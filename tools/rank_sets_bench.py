"""Time of the filtered ranking metrics (evaluation.eval_rank_queries with known_answers = the device index: filtered MRR and
hits@k over ALL entities of each query's target mode) over test sets sampled on the device index, three ways:

  list   the sets through QuerySet.queries() -- one graph.Query per query -- then the list route: per formula and batch
         index.answers, rank_targets (ids translated on the host, the bitmaps compacted to a CSR with a synchronising read)
         and a copy of the ranks. queries() is timed apart (queries_ms) and included in ms.
  sets   the QuerySets themselves: per formula and window index.answers over the device ids and rank_ids
  mixed  kg.MixedQuerySet.from_sets(sets), built once outside the rounds: per window of a query type's concatenation
         index.records_of_ids + index.answers_mixed and ONE rank_ids_mixed call -- one embedding call and one
         mpqe_rank_entities_mixed over the window's target modes, the answers' bitmaps as the exclusion words

on the `small` (480 entities) and `aifb` (2 601 entities) synthetic shapes of tools/eval_sets_bench.py, for both models. The
sides run in the same process in alternating rounds after --warmup rounds of each; a round's time is the host clock around
the call (the ranks' copy to the host and the error-word read included), ending in a device synchronise. Medians of
--rounds rounds, min and max beside them; the three sides must return the same dict (checked every round).

  kernels   one window of --batch-size queries against ONE table of the `aifb` shape's widest mode: mpqe_rank_entities
            (ops.rank_entities) beside mpqe_rank_entities_mixed with one set (ops.rank_entities_mixed) -- the plan launch
            and the permuted reads are the difference --, device events around blocks of calls, allocation included

    python tools/rank_sets_bench.py [--kgs small aifb] [--models rgcn gqe] [--per-type 256] [--out profiles/rank_sets_bench.json]
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


def stats(ms):
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def run(kg, which, args, device, emit):
    import eval_sets_bench as esb
    import kg_answers_bench as kab
    from mpqe_amd import evaluation, ops
    from mpqe_amd.kg import MixedQuerySet
    model, index, sets = esb.build(kg, which, args, device)
    order = []
    for f in sets:
        if f.query_type not in order:
            order.append(f.query_type)
    sets = {f: qs for qt in order for f, qs in sets.items() if f.query_type == qt}       # (the mixed route's order)
    mixed = MixedQuerySet.from_sets(sets)
    Q = sum(len(qs) for qs in sets.values())
    windows = sum(-(-len(ms) // args.batch_size) for ms in mixed.values())
    per_window = [len(set(ms.formula_of_host[lo:lo + args.batch_size].tolist()))
                  for ms in mixed.values() for lo in range(0, len(ms), args.batch_size)]
    base = dict(kg=kg, model=which, queries=Q, formulas=len(sets), windows=windows,
                formulas_per_window=float(np.mean(per_window)), batch_size=args.batch_size, embed_dim=args.embed_dim)
    last = {}

    def timed(name, what, prepare=None):
        def side():
            t0 = time.perf_counter()
            arg = prepare() if prepare else what
            t1 = time.perf_counter()
            out = evaluation.eval_rank_queries(arg, model, batch_size=args.batch_size, known_answers=index)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            last[name] = out
            return [1e3 * (t2 - t0), 1e3 * (t1 - t0)]
        return side
    sides = {'list': timed('list', None, lambda: {f: qs.queries() for f, qs in sets.items()}),
             'sets': timed('sets', sets), 'mixed': timed('mixed', mixed)}
    with torch.no_grad():
        for _ in range(args.warmup):
            for side in sides.values():
                side()
        times = {side: [] for side in sides}
        for _ in range(args.rounds):                    # alternating: the sides see the same machine
            for name, side in sides.items():
                times[name].append(side())
            if not (last['list'] == last['sets'] == last['mixed']):
                raise SystemExit('rank_sets_bench: the routes disagree on %s / %s' % (kg, which))
    index.check()
    for side in sides:
        t = np.asarray(times[side])
        emit(dict(base, row=side, ms=stats(t[:, 0]), queries_ms=stats(t[:, 1]), mrr=last[side]['mrr'],
                  hits10=last[side].get('hits@10')))
    if (kg, which) != (args.kgs[-1], args.models[-1]):
        return
    # one single-table window through both entries
    mode = max(index.modes, key=lambda m: index.mode_rows[index.mode_index[m]])
    n = int(index.mode_rows[index.mode_index[mode]])
    table = model.enc.table(mode).detach()[:n]
    g = torch.Generator(device='cpu').manual_seed(args.seed)
    B = args.batch_size
    q = torch.randn(B, table.shape[1], generator=g).to(device)
    target = torch.randint(0, n, (B,), generator=g).to(device)
    group = torch.zeros(B, dtype=torch.int64, device=device)
    bits = torch.zeros((B, (n + 31) // 32), dtype=torch.int32, device=device)      # (exclusion words that exclude nothing)
    desc = ops.RankMixedDescriptors([table], [0])
    err = ops.new_error_word(device)
    emit(dict(row='kernels', rows=n, batch_size=B, embed_dim=int(table.shape[1]),
              rank_entities_ms=kab.event_timed(lambda: ops.rank_entities(q, table, target, None, 0, err=err),
                                               args.warmup, args.rounds),
              rank_entities_mixed_ms=kab.event_timed(lambda: ops.rank_entities_mixed(q, desc, group, target, bits, 0, err=err),
                                                     args.warmup, args.rounds)))
    ops.raise_on_flags(err)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--kgs', nargs='+', default=['small', 'aifb'])
    ap.add_argument('--models', nargs='+', default=['rgcn', 'gqe'])
    ap.add_argument('--per-type', type=int, default=256, help='test queries per query type')
    ap.add_argument('--min-per-formula', type=int, default=1)
    ap.add_argument('--neg-max', type=int, default=100)
    ap.add_argument('--batch-size', type=int, default=128)
    ap.add_argument('--embed-dim', type=int, default=64)
    ap.add_argument('--degree', type=int, default=2)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('rank_sets_bench: needs the GPU (a CPU timing says nothing about it)')
    device = torch.device('cuda:0')
    rows = []

    def emit(r):
        rows.append(r)
    for kg in args.kgs:
        for which in args.models:
            run(kg, which, args, device, emit)
    print('| kg | model | queries | formulas | formulas / window | list ms (of which queries()) | sets ms | mixed ms [min .. max] | '
          'list / mixed | sets / mixed |', file=sys.stderr)
    print('|---|---|---:|---:|---:|---:|---:|---:|---:|---:|', file=sys.stderr)
    keyed = {}
    for r in rows:
        if r['row'] != 'kernels':
            keyed.setdefault((r['kg'], r['model']), {})[r['row']] = r
    for (kg, which), d in keyed.items():
        li, se, mi = d['list'], d['sets'], d['mixed']
        print('| %s | %s | %d | %d | %.1f | %.1f (%.1f) | %.1f | %.1f [%.1f .. %.1f] | %.1fx | %.1fx |'
              % (kg, which, li['queries'], li['formulas'], li['formulas_per_window'], li['ms'][0], li['queries_ms'][0],
                 se['ms'][0], mi['ms'][0], mi['ms'][1], mi['ms'][2], li['ms'][0] / mi['ms'][0], se['ms'][0] / mi['ms'][0]),
              file=sys.stderr)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(dict(args=vars(args), rows=rows), f, indent=1)
    print(json.dumps(dict(tool='rank_sets_bench', rows=rows)))          # the one JSON line
    return rows


if __name__ == '__main__':
    main()
